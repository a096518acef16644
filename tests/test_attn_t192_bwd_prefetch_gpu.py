"""attn_t192_bwd with the next head's rows fetched by the DMA waves (m3l_set_attn_t192_bwd_prefetch(1)) against the body in which every
compute wave loads its own rows (mode 0, the code the float64 slice tests and the parity suites have held so far): the same instructions on
the same operands in the same order, so every comparison here is on bits, with no tolerance.

The launcher is called directly through its mangled name, as tools/t192_probe.py does.  Shapes: both widths; B = 3 with a single token, the
edges of a 16-token wave tile, whole waves past n, a ragged last wave and the full 192; B = 260 > the number of CUs."""
import ctypes as C

import pytest
import torch

pytestmark = pytest.mark.gpu

from m3l_amd import Transformer  # noqa: E402
from m3l_amd import _lib as L  # noqa: E402

DEV = "cuda:0"
SYM = "_Z17m3l_attn_t192_bwdiiiPKvS0_S0_PKfS0_PvP12ihipStream_t"


def _problem(D, B, n, seed, scale=1.0):
    """random bf16 dx1_t, qkv, o, woT and a positive lse"""
    g = torch.Generator(device=DEV).manual_seed(seed)
    rn = lambda *s, sc=1.0: torch.randn(*s, device=DEV, generator=g) * sc  # noqa: E731
    bf = torch.bfloat16
    M, H = B * n, D // 64
    return dict(D=D, B=B, n=n, dxt=rn(M, D, sc=scale).to(bf), qkv=rn(M, 3 * D, sc=scale).to(bf), o=rn(M, D, sc=scale).to(bf),
                lse=rn(B * H * n).abs() + 3.0, woT=rn(D, D, sc=0.05 * scale).to(bf))


def _launch(p, mode, fill=0xFF):
    """dqkv [B n, 3 D] of one launch in `mode`, as int16 bit patterns; the buffer holds `fill` bytes before the launch"""
    lib = L.lib()
    P = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
    dqkv = torch.empty(p["B"] * p["n"], 3 * p["D"], device=DEV, dtype=torch.bfloat16)
    dqkv.view(torch.uint8).fill_(fill)
    old = lib.m3l_set_attn_t192_bwd_prefetch(mode)
    try:
        rc = getattr(lib, SYM)(p["D"], p["B"], p["n"], P(p["dxt"]), P(p["qkv"]), P(p["o"]), P(p["lse"]), P(p["woT"]), P(dqkv),
                               C.c_void_p(torch.cuda.current_stream().cuda_stream))
        torch.cuda.synchronize()
    finally:
        lib.m3l_set_attn_t192_bwd_prefetch(old)
    assert rc == 0
    return dqkv.view(torch.int16).clone(), bool(torch.isfinite(dqkv.float()).all())


@pytest.mark.parametrize("D", [192, 256])
@pytest.mark.parametrize("B,n", [(3, 1), (3, 16), (3, 17), (3, 49), (3, 130), (3, 177), (3, 191), (3, 192), (260, 192)])
def test_prefetch_is_bit_identical(D, B, n):
    p = _problem(D, B, n, seed=1000 * D + n)
    ref, fin0 = _launch(p, 0)
    new, fin1 = _launch(p, 1)
    assert fin0 and fin1
    assert torch.equal(ref, new)


@pytest.mark.parametrize("D", [192, 256])
def test_prefetch_ignores_stale_memory(D):
    """what an earlier launch left in LDS and what the output buffer held before do not reach the result: a problem with whole waves and part
    of a wave past n, then a full-length one with large values, then the first again over 0xFF bytes and over zeros"""
    p = _problem(D, 3, 130, seed=D)
    big = _problem(D, 3, 192, seed=D + 1, scale=40.0)
    ref, fin = _launch(p, 0)
    first, fin1 = _launch(p, 1)
    assert fin and fin1 and torch.equal(ref, first)
    _launch(big, 1)
    again_ff, fin_ff = _launch(p, 1, fill=0xFF)
    _launch(big, 1)
    again_00, fin_00 = _launch(p, 1, fill=0x00)
    assert fin_ff and fin_00
    assert torch.equal(first, again_ff) and torch.equal(first, again_00)


def test_prefetch_through_the_module():
    """a 2-layer decoder-shaped stack, row-tile family forced: forward + backward in both modes, every gradient bit-identical"""
    torch.manual_seed(7)
    tf = Transformer(192, 2, 3, 64, 768)
    tf.compute_dtype = "bf16"
    tf = tf.to(DEV)
    g = torch.Generator().manual_seed(8)
    x = (torch.randn(3, 192, 192, generator=g) * 1.5).to(DEV)
    cot = torch.randn(3, 192, 192, generator=g).to(DEV)
    lib = L.lib()
    res = {}
    old_t192 = lib.m3l_set_t192(7)
    try:
        for mode in (0, 1):
            old = lib.m3l_set_attn_t192_bwd_prefetch(mode)
            try:
                tf.zero_grad(set_to_none=True)
                xg = x.clone().requires_grad_(True)
                (tf(xg) * cot).sum().backward()
                torch.cuda.synchronize()
            finally:
                lib.m3l_set_attn_t192_bwd_prefetch(old)
            res[mode] = (xg.grad.clone(), {k: q.grad.clone() for k, q in tf.named_parameters()})
    finally:
        lib.m3l_set_t192(old_t192)
    assert torch.isfinite(res[1][0]).all()
    assert torch.equal(res[0][0], res[1][0])
    for k in res[0][1]:
        assert torch.equal(res[0][1][k], res[1][1][k]), k
