"""The attention backward block with all heads of a sample in one pass (attn_block_bwd_allheads_body, m3l_set_attn_bwd_heads(1)) against
the body that takes one head after the other (mode 0): the same instructions on the same operands in the same order, so the input
gradient and every parameter gradient must be bit-identical (torch.equal, no tolerance) — per residual-stream type, per launch shape of
the backward (one launch per half layer / one per weight-gradient group), at every row-tile count, in both branches of the task list
(one task per wave; dQ then dK / dV on one wave at H = 3, n > 32), at KT = 2 and with more workgroups than CUs.

The all-heads body writes dq, dk, dv over the q, k, v tiles it holds in LDS and keeps no image of dx1_t or o there: the last test holds
it to the same bits whatever LDS and its output buffers held before."""
import pytest
import torch

pytestmark = pytest.mark.gpu

from m3l_amd import Transformer  # noqa: E402
from m3l_amd import _lib as L  # noqa: E402
from m3l_amd import functional as Fn  # noqa: E402

DEV = "cuda:0"

# (D, heads, mlp, n, B, depth)
SHAPES = [(192, 3, 768, n, 3, 2) for n in (1, 15, 16, 17, 32, 33, 47, 48)]          # every RT, both task-list branches, tile edges
SHAPES += [(128, 2, 256, n, 5, 3) for n in (1, 17, 33, 48)]                          # KT = 2
SHAPES += [(192, 3, 768, 48, 260, 1)]                                                # more workgroups than CUs


def _stack(D, heads, mlp, n, B, depth, seed=0):
    torch.manual_seed(D + n + seed)
    tf = Transformer(D, depth, heads, 64, mlp)
    tf.compute_dtype = "bf16"
    tf = tf.to(DEV)
    g = torch.Generator().manual_seed(n + seed)
    x = (torch.randn(B, n, D, generator=g) * 1.5).to(DEV)
    cot = torch.randn(B, n, D, generator=g).to(DEV)
    return tf, x, cot


def _run(tf, x, cot, heads_mode, rb, mega):
    lib = L.lib()
    old = (lib.m3l_set_attn_block(3), lib.m3l_set_residual_bf16(rb), lib.m3l_set_enc_mega(mega), lib.m3l_set_attn_bwd_heads(heads_mode))
    try:
        tf.zero_grad(set_to_none=True)
        xg = x.clone().requires_grad_(True)
        y = tf(xg)
        (y * cot).sum().backward()
        torch.cuda.synchronize()
    finally:
        lib.m3l_set_attn_bwd_heads(old[3])
        lib.m3l_set_enc_mega(old[2])
        lib.m3l_set_residual_bf16(old[1])
        lib.m3l_set_attn_block(old[0])
    return y.detach().cpu(), xg.grad.cpu(), {k: p.grad.cpu().clone() for k, p in tf.named_parameters()}


def _same(a, b, what):
    assert torch.equal(a[0], b[0]), (what, "y")
    assert torch.equal(a[1], b[1]), (what, "dx")
    for k in a[2]:
        assert torch.equal(a[2][k], b[2][k]), (what, k)


@pytest.mark.parametrize("rb", [0, 1])
@pytest.mark.parametrize("D,heads,mlp,n,B,depth", SHAPES)
def test_all_heads_backward_is_bit_identical_to_per_head(D, heads, mlp, n, B, depth, rb):
    tf, x, cot = _stack(D, heads, mlp, n, B, depth)
    for mega in ((0, 1, 3) if rb == 0 else (0, 1)):          # (the grouped backward launch, bit 2, runs the fp32 residual stream only)
        ref = _run(tf, x, cot, 0, rb, mega)
        new = _run(tf, x, cot, 1, rb, mega)
        assert bool(torch.isfinite(new[1]).all())
        _same(ref, new, (mega, rb))


@pytest.mark.parametrize("n", [17, 33])
def test_all_heads_backward_ignores_stale_memory(monkeypatch, n):
    """First run in fresh buffers; then a backward of another length with other values (what LDS holds afterwards), then the first
    problem again with every workspace — dqkv's backing store among them — pre-filled with NaN (0xFF) and with zeros: the same bits."""
    tf, x, cot = _stack(192, 3, 768, n, 3, 2)
    first = _run(tf, x, cot, 1, 1, 1)
    tf2, x2, cot2 = _stack(192, 3, 768, 48, 3, 2, seed=5)
    _run(tf2, x2 * 40.0, cot2 * 1e3, 1, 1, 1)
    for fill in (0xFF, 0x00):
        monkeypatch.setattr(Fn, "_ws", lambda nbytes, device, fill=fill: torch.full((int(nbytes),), fill, dtype=torch.uint8, device=device))
        again = _run(tf, x, cot, 1, 1, 1)
        assert bool(torch.isfinite(again[1]).all()) and all(bool(torch.isfinite(v).all()) for v in again[2].values())
        _same(first, again, ("stale", fill))
