"""The fc2 weight gradient of a stack that did not save h (wgrad.hip, TnProblem::gelu_x): dW = Y^T GELU(u) with the GELU applied to the
staged operand in LDS, through m3l_op_gemm_tn_grouped_gelu and the plan query m3l_op_gemm_tn_grouped_plan.

  * the ways of applying it — every wave on its own pieces one ring stage ahead (m3l_set_wgrad_gelu_ahead(1)), the same with the middle
    wave of each SIMD converting before it multiplies (2), and the earlier all-wave pass with its second barrier (0) — give the same bits;
  * they agree with float64 Y^T GELU_erf(u) within the rounding of h to bf16 plus the fitted form's stated error;
  * a group whose gelu_x are all zero is m3l_op_gemm_tn_grouped bit for bit.

Problem lists and M values are chosen with the plan query so that both tile families, GELU on the wide and on the narrow operand, one and
several row ranges, and per-range stage counts 1, 2, 3 (= ring depth - 1), 4 and >= 6 with a ragged last stage all occur; the coverage
is asserted, not assumed (test_the_lists_cover_the_kernels_cases runs without a GPU)."""
import ctypes as C
import functools
import math

import pytest
import torch

from m3l_amd import _lib as L

# (N, K, gelu on X): dW [N, K] = Y^T X with Y [M, N], X [M, K]
LAYER = [(576, 192, 0), (192, 192, 0), (768, 192, 0), (192, 768, 1)]           # ViT-Tiny: qkv, out-proj, fc1, fc2 (X = u)
LISTS = {
    "fc2": [(192, 768, 1)],                 # X wide: the GELU operand is the wide one
    "narrow": [(768, 192, 1)],              # X narrow
    "conv": [(192, 32, 1)],                 # a 256-wide tile, X narrow
    "conv_t": [(32, 192, 1)],               # ... X wide
    "layer": LAYER,
    "layers2": LAYER + LAYER,
}
TILES = {"fc2": (6, 3), "narrow": (6, 3), "layer": (6, 3), "layers2": (6, 3)}    # 384 x 192; the conv shapes: 256 wide
MS = (1, 33, 64, 96, 128, 200, 2100)
PLANTED = (0.0, -0.0, 8.0, -8.0, 8.5, -8.5, 12.0, -12.0, 4e-40)                  # the clamp of gelu_fast_sig is at |x| = 8; a bf16 denormal


def wplan(probs, M):
    n = len(probs)
    N, K = (C.c_int * n)(*[p[0] for p in probs]), (C.c_int * n)(*[p[1] for p in probs])
    o = [C.c_int() for _ in range(4)]
    L.check(L.lib().m3l_op_gemm_tn_grouped_plan(n, M, N, K, *[C.byref(v) for v in o]), "m3l_op_gemm_tn_grouped_plan")
    return tuple(v.value for v in o)            # na, tbt, nsplit, rows_per_split


def stage_counts(M, nsplit, rps):
    return [math.ceil(min(rps, M - s * rps) / 32) for s in range(nsplit)]


def test_the_lists_cover_the_kernels_cases():
    assert 1 in MS and any(m % 32 for m in MS)
    for name, probs in LISTS.items():
        seen, multi, ragged = set(), False, False
        for M in MS:
            na, tbt, S, rps = wplan(probs, M)
            if name in TILES:
                assert (na, tbt) == TILES[name], (name, M, na, tbt)
            else:
                assert na == 4 and tbt in (2, 3, 4), (name, M, na, tbt)
            assert rps % 64 == 0 and (S - 1) * rps < M <= S * rps
            seen |= set(stage_counts(M, S, rps))
            multi |= S > 1
            ragged |= any(min(rps, M - s * rps) % 32 for s in range(S))
        assert {1, 2, 3, 4} <= seen and max(seen) >= 6 and multi and ragged, (name, sorted(seen), multi, ragged)


@functools.lru_cache(maxsize=None)
def inputs(name, M):
    """bf16 operands of a list at M rows (CPU, made once): Y ~ N(0, 1); X ~ N(0, 2^2) with the planted values spread over it"""
    g = torch.Generator().manual_seed(1000 * sorted(LISTS).index(name) + M)
    out = []
    for N, K, _ in LISTS[name]:
        Y = torch.randn(M, N, generator=g).bfloat16()
        X = (2.0 * torch.randn(M, K, generator=g)).bfloat16()
        flat = X.view(-1)
        pos = torch.linspace(0, flat.numel() - 1, len(PLANTED)).long()
        assert len(set(pos.tolist())) == len(PLANTED)
        flat[pos] = torch.tensor(PLANTED, dtype=torch.float64).to(torch.bfloat16)
        assert float(flat[pos[-1]].float()) != 0.0 and abs(float(flat[pos[-1]].float())) < 1.2e-38, "the denormal survived the cast"
        out.append((Y, X))
    return out


@functools.lru_cache(maxsize=None)
def reference(name, M):
    """per GELU problem: float64 Y^T GELU_erf(u), |Y|^T |h| and the column mass |Y|^T 1"""
    ref = []
    for (N, K, gx), (Y, X) in zip(LISTS[name], inputs(name, M)):
        if not gx:
            ref.append(None)
            continue
        y, u = Y.double(), X.double()
        h = 0.5 * u * (1.0 + torch.erf(u / math.sqrt(2.0)))
        ref.append((y.t() @ h, y.abs().t() @ h.abs(), y.abs().sum(0)))
    return ref


def run(name, M, form, ahead, entry="gelu"):
    """the grouped launch on the device; `form` replaces the 1 of the list's gelu flags (0: none).  Returns the dW list (CPU, fp32)"""
    lib, probs, dev = L.lib(), LISTS[name], torch.device("cuda:0")
    n = len(probs)
    ten = [(Y.to(dev), X.to(dev)) for Y, X in inputs(name, M)]
    outs = [torch.full((N, K), float("nan"), device=dev) for N, K, _ in probs]
    N, K = (C.c_int * n)(*[p[0] for p in probs]), (C.c_int * n)(*[p[1] for p in probs])
    gx = (C.c_int * n)(*[form if p[2] else 0 for p in probs])
    ws_bytes = lib.m3l_op_gemm_tn_grouped_ws_bytes(1, n, M, N, K)
    ws = torch.empty(ws_bytes // 4 + 64, device=dev)
    st = torch.cuda.current_stream().cuda_stream
    args = [1, n, M, L.ptr_array([t[0] for t in ten]), N, L.ptr_array([t[1] for t in ten]), K, N, K, L.ptr_array(outs), L.ptr(ws), ws_bytes]
    old = lib.m3l_set_wgrad_gelu_ahead(ahead)
    try:
        if entry == "gelu":
            L.check(lib.m3l_op_gemm_tn_grouped_gelu(*args, gx, st), "m3l_op_gemm_tn_grouped_gelu")
        else:
            L.check(lib.m3l_op_gemm_tn_grouped(*args, st), "m3l_op_gemm_tn_grouped")
        torch.cuda.synchronize()
    finally:
        lib.m3l_set_wgrad_gelu_ahead(old)
    return [o.cpu() for o in outs]


@pytest.mark.gpu
@pytest.mark.parametrize("form", [1, 2], ids=["erf", "fitted"])
@pytest.mark.parametrize("name", sorted(LISTS))
def test_ahead_and_pass_are_bit_identical_and_match_float64(name, form):
    for M in MS:
        a, b, c = run(name, M, form, 1), run(name, M, form, 0), run(name, M, form, 2)
        for i, (x, y, z) in enumerate(zip(a, b, c)):
            assert torch.isfinite(x).all(), (name, M, i)
            assert torch.equal(x, y), f"{name} M={M} problem {i}: the two GELU modes differ in {int((x != y).sum())} elements"
            assert torch.equal(x, z), f"{name} M={M} problem {i}: the alternating order differs in {int((x != z).sum())} elements"
        for i, r in enumerate(reference(name, M)):
            if r is None:
                continue
            ref, mass_h, mass_1 = r
            err = (a[i].double() - ref).abs()
            bound = 2.0 ** -8 * mass_h + 1.2e-4 * mass_1[:, None]
            worst = float((err / bound.clamp_min(1e-300)).max())
            print(f"{name} M={M} form={form} problem {i}: max err {float(err.max()):.3e}, worst err/bound {worst:.3f}")
            assert bool((err <= bound).all()), f"{name} M={M} problem {i}: err/bound {worst:.3f}"


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(LISTS))
def test_a_group_without_gelu_is_the_plain_grouped_launch(name):
    for M in MS:
        a, b = run(name, M, 0, 1), run(name, M, 0, 1, entry="plain")
        for i, (x, y) in enumerate(zip(a, b)):
            assert torch.isfinite(x).all() and torch.equal(x, y), (name, M, i)
