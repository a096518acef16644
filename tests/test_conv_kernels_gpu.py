"""The EarlyCNN stem's convolution kernels one by one, through the m3l_op_conv_* / m3l_op_im2col / m3l_op_col2im_relu exports, against the
float64 restatement of tests/conv_refs.py (anchored by tests/test_conv_refs_cpu.py).  Needs the MI355X.

Kernels: conv_prep_kernel, conv_fwd_kernel, conv_wgrad_kernel (+ the slab reduce), conv_dgrad_kernel of conv.hip; im2col_kernel<T>,
im2col4_bf16_kernel, col2im_relu_kernel<T> of elementwise.hip.  Every output and the weight-gradient slab is a NaN-filled
[guard | payload | guard] block of tests/memguard.py; the guards are checked after the launches.

Layer shapes: the (Ci, Co) of the stems of dim 64 / 128 / 192 / 256.  Eleven of the twelve have direct kernels; the third layer of
dim 192, (48, 96), has none — Ci = 48 is three 16-channel tiles, Co = 96 eight, and conv.hip has no (8, 3) weight-gradient template — so
its exports must refuse it (test_dim192_third_layer_has_no_direct_kernel) and the dim-192 stem as a whole runs im2col + GEMM, which the
stem-level test pins bit for bit.  (12, 24) and (24, 48) still reach the partial accumulator tiles (Co = 24 / 48 against 32 / 64 rows) and
the padded NHWC input (Ci = 24 in 32 LDS channels).

Exact cases (the main check): inputs and dY integers in [-3, 3], weights integers in [-2, 2], bias integers, act with positives, exact
zeros, -0.0 and negatives.  Every sum is an integer below 2^24 in magnitude (forward <= 16 * 64 * 6 + |bias|, weight gradient
<= 9 B OH OW, input gradient <= 9 * 128 * 6), so any fp32 accumulation order is exact and the result must equal the float64 result —
dW (f32) as it is, out / dX (bf16) after one round-to-nearest-even.  torch.equal, no tolerance.

General-valued cases, one per template and kind: N(0,1) operands rounded to bf16 first; per element |H - X| <= 2 n u sum|terms| for f32
outputs and + 2^-8 |X| for bf16 outputs (u = 2^-24, n = the number of terms of that element's sum, which bounds any summation order; 2 is
the margin of test_replay_per_gpu.py; 2^-8 one bf16 rounding).  The worst fraction of the bound is printed per kernel at the end of the
module (recorded in EXPERIMENTS.md).

Weight gradient with tiles_per_wg >= 2: one case per conv_wgrad_kernel template (MT, NT) in {(1,1), (2,1), (4,2), (8,4)} and kind, with
more tiles than groups max(128, 2^24 / (Co Ci k k)) and a tile count that is no multiple of tiles_per_wg (the last workgroup is short).
The (1,1) template runs at (8, 16); the other (1,1) pairs need more: (3, 8) 43 691 tiles (134 MB of input), (6, 16) 10 923.  The loop is the
same code for every pair of a template.
"""
import ctypes as C

import pytest
import torch

import conv_refs as R
from memguard import MemGuard

pytestmark = pytest.mark.gpu

from m3l_amd import _lib as L  # noqa: E402
from m3l_amd import functional as Fn  # noqa: E402

F64 = torch.float64
BF16 = torch.bfloat16
U = 2.0 ** -24
WORST = {}      # kernel -> worst fraction of its bound over the general-valued cases


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    L.lib()
    yield torch.device("cuda:0")
    for k, v in sorted(WORST.items()):
        print(f"[conv worst] {k:22s} fraction of the bound = {v:.3g}")


def _guard():
    return MemGuard(None, 0xFF, callers="all", tensor_guard=4096)


def _srcs(x):
    return L.ptr_array(x if isinstance(x, list) else [x])


def _geom(x):
    """(nsrc, nchw, Bsrc, Ci, H, W) of a list of NCHW f32 sources or of one NHWC tensor"""
    if isinstance(x, list):
        Bs, Ci, H, W = x[0].shape
        return len(x), 1, Bs, Ci, H, W
    B, H, W, Ci = x.shape
    return 1, 0, B, Ci, H, W


# ---- launches: each returns guarded, NaN-filled outputs
def run_prep(g, dev, w, KH, S, want_wd):
    Co, Ci = w.shape[:2]
    wf_b, wd_b, _ = R.sizes(1, Ci, 8, 8, Co, KH, S, 1)
    Wf = g.alloc((16 * R.mt_of(Co), wf_b // (32 * R.mt_of(Co))), BF16, dev)
    Wd = g.alloc(((4 if S == 2 else 1), R.pad16(Ci), (4 if S == 2 else KH * KH) * Co), BF16, dev) if want_wd else None
    assert Wf.numel() * 2 == wf_b and (Wd is None or Wd.numel() * 2 == wd_b)
    L.check(L.lib().m3l_op_conv_prep(L.ptr(w), Ci, Co, KH, S, L.ptr(Wf), L.ptr(Wd), Fn._stream()), "m3l_op_conv_prep")
    return Wf, Wd


def run_fwd(g, dev, x, Co, KH, S, P, Wf, bias):
    nsrc, nchw, Bs, Ci, H, W = _geom(x)
    OH, OW = R.out_size(H, W, KH, S, P)
    out = g.alloc((nsrc * Bs, OH, OW, Co), BF16, dev)
    L.check(L.lib().m3l_op_conv_fwd(_srcs(x), nsrc, nchw, Bs, Ci, H, W, Co, KH, S, P, L.ptr(Wf), L.ptr(bias), L.ptr(out), Fn._stream()), "m3l_op_conv_fwd")
    return out


def run_wgrad(g, dev, x, dY, KH, S, P):
    nsrc, nchw, Bs, Ci, H, W = _geom(x)
    Co = dY.shape[3]
    slab_b = R.sizes(nsrc * Bs, Ci, H, W, Co, KH, S, P)[2]
    got = C.c_size_t(0)
    assert L.lib().m3l_op_conv_sizes(nsrc * Bs, Ci, H, W, Co, KH, S, P, None, None, C.byref(got)) == 0 and got.value == slab_b
    slab = g.alloc((slab_b // 4,), torch.float32, dev)
    dW = g.alloc((Co, Ci, KH, KH), torch.float32, dev)
    L.check(L.lib().m3l_op_conv_wgrad(_srcs(x), nsrc, nchw, Bs, Ci, H, W, Co, KH, S, P, L.ptr(dY), L.ptr(slab), L.ptr(dW), Fn._stream()), "m3l_op_conv_wgrad")
    return dW


def run_dgrad(g, dev, dY, Ci, H, W, KH, S, P, Wd, act):
    B, _, _, Co = dY.shape
    dX = g.alloc((B, H, W, Ci), BF16, dev)
    L.check(L.lib().m3l_op_conv_dgrad(L.ptr(dY), B, Ci, H, W, Co, KH, S, P, L.ptr(Wd), L.ptr(act), L.ptr(dX), Fn._stream()), "m3l_op_conv_dgrad")
    return dX


def run_im2col(g, dev, dt, x, KH, S, P, Kpad):
    nsrc, nchw, Bs, Ci, H, W = _geom(x)
    OH, OW = R.out_size(H, W, KH, S, P)
    col = g.alloc((nsrc * Bs * OH * OW, Kpad), BF16 if dt else torch.float32, dev)
    L.check(L.lib().m3l_op_im2col(dt, _srcs(x), nsrc, nchw, Bs, Ci, H, W, KH, S, P, Kpad, L.ptr(col), Fn._stream()), "m3l_op_im2col")
    return col


def run_col2im(g, dev, dt, dcol, B, Ci, H, W, KH, S, P, act):
    dX = g.alloc((B, H, W, Ci), BF16 if dt else torch.float32, dev)
    L.check(L.lib().m3l_op_col2im_relu(dt, L.ptr(dcol), B, Ci, H, W, KH, S, P, dcol.shape[1], L.ptr(act), L.ptr(dX), Fn._stream()), "m3l_op_col2im_relu")
    return dX


# ---- checks
def check_equal(what, H, X):
    """H equals the float64 result X after one rounding to H's type (exact for f32: X is an integer below 2^24)"""
    Hc, want = H.detach().cpu(), X.to(torch.float32).to(H.dtype)
    if not torch.equal(Hc, want):
        bad = torch.nonzero(Hc.float() != want.float())          # NaN != anything: poison that was left shows up here
        raise AssertionError(f"{what}: {bad.shape[0]} of {Hc.numel()} elements differ; first at {bad[:8].tolist()}: got "
                             f"{[float(Hc[tuple(i)]) for i in bad[:8]]}, want {[float(want[tuple(i)]) for i in bad[:8]]}")


def check_bound(kernel, what, H, X, mag, n):
    """|H - X| <= 2 n u sum|terms| (+ 2^-8 |X| for a bf16 output), per element"""
    Hd = H.detach().to("cpu", F64)
    bound = 2.0 * n * U * mag + (2.0 ** -8 * X.abs() if H.dtype == BF16 else 0.0)
    err = (Hd - X).abs()
    assert bool(torch.isfinite(Hd).all()), f"{kernel} {what}: non-finite output"
    frac = float(torch.where(bound > 0, err / bound.clamp_min(1e-300), torch.where(err > 0, torch.full_like(err, float("inf")), torch.zeros_like(err))).max())
    WORST[kernel] = max(WORST.get(kernel, 0.0), frac)
    print(f"[conv] {kernel} {what}: fraction of the bound = {frac:.3g}")
    assert frac <= 1.0, f"{kernel} {what}: {frac:.3g} of the bound"


# ---- data
def _ints(g, shape, lo, hi):
    return torch.randint(lo, hi + 1, shape, generator=g).float()


def _neg_zeros(t, g):
    """half of the exact zeros become -0.0"""
    flip = (t == 0) & (torch.rand(t.shape, generator=g) < 0.5)
    return torch.where(flip, torch.full_like(t, -0.0), t)


def layer_data(dev, Ci, Co, kind, hw, batch, exact, seed):
    """batch: B of an NHWC input, or (nsrc, Bsrc) of NCHW f32 sources.  Returns device tensors x, w, bias, dY, act and their CPU copies."""
    KH, S, P = R.KINDS[kind]
    H, W = hw
    g = torch.Generator().manual_seed(seed)
    draw = (lambda shape, lo, hi: _ints(g, shape, lo, hi)) if exact else (lambda shape, lo, hi: torch.randn(shape, generator=g).to(BF16).float())
    if isinstance(batch, tuple):
        x = [draw((batch[1], Ci, H, W), -3, 3) for _ in range(batch[0])]
        B = batch[0] * batch[1]
    else:
        x = _neg_zeros(draw((batch, H, W, Ci), -3, 3), g).to(BF16)
        B = batch
    OH, OW = R.out_size(H, W, KH, S, P)
    w = draw((Co, Ci, KH, KH), -2, 2)
    bias = _ints(g, (Co,), -4, 4) if exact else torch.randn(Co, generator=g)
    dY = draw((B, OH, OW, Co), -3, 3).to(BF16)
    act = _neg_zeros(draw((B, H, W, Ci), -3, 3), g).to(BF16)
    cpu = dict(x=x, w=w, bias=bias, dY=dY, act=act)
    d = {k: ([t.to(dev) for t in v] if isinstance(v, list) else v.to(dev)) for k, v in cpu.items()}
    return d, cpu, (KH, S, P, H, W, OH, OW, B)


def _has_dgrad(first, Co, KH, S):
    return not first and ((4 if S == 2 else KH * KH) * Co) % 32 == 0


S2_GEOS = [(16, 16), (20, 36), (36, 20), (6, 34), (2, 4)]       # one full tile; 2 x 3 ragged tiles; its transpose; one ragged tile row; 1 x 2 output
S2_DGRAD_GEOS = [(34, 18)]                                       # input tiles of 16: 3 x 2, ragged both ways ((20, 36) is in the list above)
K3_GEOS = [(8, 8), (10, 18), (18, 10), (3, 6), (1, 2)]
FIRST = [(3, 8), (6, 16), (12, 24), (12, 32)]                    # NCHW f32 first layers, 4x4 / 2 / 1
LATER = [(8, 16, 0), (24, 48, 0), (16, 32, 0), (16, 32, 1), (32, 64, 0), (32, 64, 1), (64, 128, 0), (64, 128, 1)]     # NHWC: (Ci, Co, kind)
EXACT_CASES = [(Ci, Co, 0, hw, batch) for Ci, Co in FIRST for hw in S2_GEOS for batch in ((3, 1), (2, 2))] + \
              [(Ci, Co, kind, hw, 3) for Ci, Co, kind in LATER for hw in (K3_GEOS if kind else S2_GEOS + S2_DGRAD_GEOS)]


@pytest.mark.parametrize("Ci,Co,kind,hw,batch", EXACT_CASES)
def test_layer_kernels_exact(dev, Ci, Co, kind, hw, batch):
    """conv_prep, conv_fwd, conv_wgrad and (behind the first layer) conv_dgrad of one layer on integer data: bit-equal to float64"""
    first = isinstance(batch, tuple)
    d, c, (KH, S, P, H, W, OH, OW, B) = layer_data(dev, Ci, Co, kind, hw, batch, True, 1000 * Ci + 10 * Co + hw[0] + 3 * hw[1])
    assert L.lib().m3l_op_conv_supported(Ci, Co, KH, S, P, int(first)) == 1
    g = _guard()
    dg = _has_dgrad(first, Co, KH, S)
    Wf, Wd = run_prep(g, dev, d["w"], KH, S, dg)
    out = run_fwd(g, dev, d["x"], Co, KH, S, P, Wf, d["bias"])
    dW = run_wgrad(g, dev, d["x"], d["dY"], KH, S, P)
    dW2 = run_wgrad(g, dev, d["x"], d["dY"], KH, S, P)
    dX = run_dgrad(g, dev, d["dY"], Ci, H, W, KH, S, P, Wd, d["act"]) if dg else None
    g.check(f"({Ci}, {Co}) kind {kind} {H} x {W}")
    check_equal("Wf", Wf, R.wf_layout(c["w"], KH))
    if dg:
        check_equal("Wd", Wd, R.wd_layout(c["w"], KH, S))
    check_equal("conv_fwd out", out, R.conv_fwd(c["x"], c["w"], c["bias"], KH, S, P))
    check_equal("conv_wgrad dW", dW, R.conv_wgrad(c["x"], c["dY"], KH, S, P))
    assert torch.equal(dW, dW2), "conv_wgrad: two runs differ"
    if dg:
        check_equal("conv_dgrad dX", dX, R.conv_dgrad(c["dY"], c["w"], c["act"], KH, S, P))


def test_dim192_third_layer_has_no_direct_kernel(dev):
    """(48, 96): (MT, NT) = (8, 3) is no template of conv.hip — every direct export refuses it with a message instead of launching; its
    arithmetic runs on the im2col path (test_lowering_kernels_exact at Ci = 48, test_stem_exact_three_paths at dim 192)"""
    lib = L.lib()
    x = torch.zeros(1, 16, 16, 48, dtype=BF16, device=dev)
    buf = torch.zeros(1 << 16, dtype=torch.float32, device=dev)
    for KH, S, P in ((4, 2, 1), (3, 1, 1)):
        assert lib.m3l_op_conv_supported(48, 96, KH, S, P, 0) == 0
        calls = (lib.m3l_op_conv_prep(L.ptr(buf), 48, 96, KH, S, L.ptr(buf), None, None),
                 lib.m3l_op_conv_fwd(_srcs(x), 1, 0, 1, 48, 16, 16, 96, KH, S, P, L.ptr(buf), L.ptr(buf), L.ptr(buf), None),
                 lib.m3l_op_conv_wgrad(_srcs(x), 1, 0, 1, 48, 16, 16, 96, KH, S, P, L.ptr(buf), L.ptr(buf), L.ptr(buf), None),
                 lib.m3l_op_conv_dgrad(L.ptr(buf), 1, 48, 16, 16, 96, KH, S, P, L.ptr(buf), L.ptr(x), L.ptr(buf), None))
        assert all(rc != 0 for rc in calls) and "no direct convolution for Ci=48 Co=96" in L.last_error()
    torch.cuda.synchronize()
    assert not buf.any()


# one per template and kind: forward MT = 1 / 2 / 4 / 8, weight gradient (MT, NT) = (1,1) / (2,1) / (4,2) / (8,4), input gradient NTI = 1 / 2 / 4;
# the NCHW loader at (3, 8) and (12, 32); the partial tiles of dim 192 at (12, 24) and (24, 48)
GENERAL_CASES = [(8, 16, 0, 3), (8, 16, 1, 3), (16, 32, 0, 3), (16, 32, 1, 3), (32, 64, 0, 3), (32, 64, 1, 3), (64, 128, 0, 3), (64, 128, 1, 3),
                 (24, 48, 0, 3), (3, 8, 0, (3, 1)), (12, 24, 0, (2, 2)), (12, 32, 0, (2, 2))]


@pytest.mark.parametrize("Ci,Co,kind,batch", GENERAL_CASES)
def test_layer_kernels_general(dev, Ci, Co, kind, batch):
    """N(0,1) operands rounded to bf16: every output within the per-element summation bound; the weight gradient the same bits twice"""
    first = isinstance(batch, tuple)
    hw = (10, 18) if kind else (20, 36)
    d, c, (KH, S, P, H, W, OH, OW, B) = layer_data(dev, Ci, Co, kind, hw, batch, False, 77 * Ci + Co + kind)
    g = _guard()
    dg = _has_dgrad(first, Co, KH, S)
    Wf, Wd = run_prep(g, dev, d["w"], KH, S, dg)
    out = run_fwd(g, dev, d["x"], Co, KH, S, P, Wf, d["bias"])
    dW = run_wgrad(g, dev, d["x"], d["dY"], KH, S, P)
    dW2 = run_wgrad(g, dev, d["x"], d["dY"], KH, S, P)
    dX = run_dgrad(g, dev, d["dY"], Ci, H, W, KH, S, P, Wd, d["act"]) if dg else None
    g.check(f"({Ci}, {Co}) kind {kind}")
    tag = f"({Ci},{Co}) k{KH}"
    check_equal("Wf", Wf, R.wf_layout(c["w"], KH))          # the operands are bf16 values: the copies are exact
    check_bound("conv_fwd", tag, out, *R.conv_fwd(c["x"], c["w"], c["bias"], KH, S, P, stats=True))
    check_bound("conv_wgrad", tag, dW, *R.conv_wgrad(c["x"], c["dY"], KH, S, P, stats=True))
    assert torch.equal(dW, dW2), "conv_wgrad: two runs differ (the slab reduce has a fixed order)"
    if dg:
        check_equal("Wd", Wd, R.wd_layout(c["w"], KH, S))
        check_bound("conv_dgrad", tag, dX, *R.conv_dgrad(c["dY"], c["w"], c["act"], KH, S, P, stats=True))


def _multi_tile_batch(Ci, Co, kind, hw):
    """the smallest batch at which the tiles exceed the groups and are no multiple of tiles_per_wg"""
    KH, S, P = R.KINDS[kind]
    B = 1
    while True:
        total, G, tpw, wgs = R.wgrad_split(B, Ci, hw[0], hw[1], Co, KH, S, P)
        if total > G and tpw >= 2 and total % tpw:
            return B, (total, G, tpw, wgs)
        B += 1


@pytest.mark.parametrize("Ci,Co,kind", [(8, 16, 0), (8, 16, 1), (16, 32, 0), (16, 32, 1), (32, 64, 0), (32, 64, 1), (64, 128, 0), (64, 128, 1)])
def test_wgrad_multi_tile_exact(dev, Ci, Co, kind):
    """conv_wgrad_kernel with tiles_per_wg >= 2 and a short last workgroup, per template and kind: the tile loop, its barrier, the
    accumulation across tiles and the t_end clamp, on integer data, bit-equal to float64 and the same bits twice.  Three tiles per image
    (output 8 x 24).  The other pairs of the (1,1) template would need more input than 64 MB ((3, 8): 43 691 tiles, 134 MB) or, at (6, 16),
    10 923 tiles of NCHW f32; their loop is this code."""
    KH, S, P = R.KINDS[kind]
    hw = (8, 24) if kind else (16, 48)
    B, (total, G, tpw, wgs) = _multi_tile_batch(Ci, Co, kind, hw)
    assert total == 3 * B and G == max(128, (1 << 24) // (Co * Ci * KH * KH)) and tpw == 2 and wgs * tpw > total and 9 * B * 8 * 24 < 2 ** 24
    assert B * hw[0] * hw[1] * Ci * 2 <= 64 << 20
    g0 = torch.Generator().manual_seed(Ci + Co + kind)
    x = torch.randint(-3, 4, (B, hw[0], hw[1], Ci), generator=g0, dtype=torch.int8)
    dY = torch.randint(-3, 4, (B, 8, 24, Co), generator=g0, dtype=torch.int8)
    xd, dYd = x.to(dev).to(BF16), dY.to(dev).to(BF16)
    g = _guard()
    dW = run_wgrad(g, dev, xd, dYd, KH, S, P)
    dW2 = run_wgrad(g, dev, xd, dYd, KH, S, P)
    g.check(f"({Ci}, {Co}) kind {kind} B {B}")
    print(f"[conv] wgrad ({Ci},{Co}) k{KH}: B={B} tiles={total} groups={G} tiles_per_wg={tpw} workgroups={wgs}")
    check_equal("conv_wgrad dW", dW, R.conv_wgrad(x, dY, KH, S, P))
    assert torch.equal(dW, dW2), "conv_wgrad: two runs differ"


# ---------------------------------------------------------------------------------------------------------------------------------
# the lowering kernels of the im2col path
LOWER_CASES = [(3, 0, hw, (3, 1)) for hw in S2_GEOS] + [(12, 0, (20, 36), (2, 2))] + \
              [(Ci, 0, hw, 3) for Ci in (8, 48) for hw in S2_GEOS + S2_DGRAD_GEOS] + [(Ci, 1, hw, 3) for Ci in (16, 48) for hw in K3_GEOS]


@pytest.mark.parametrize("Ci,kind,hw,batch", LOWER_CASES)
@pytest.mark.parametrize("dt", [0, 1], ids=["f32", "bf16"])
def test_lowering_kernels_exact(dev, dt, Ci, kind, hw, batch):
    """im2col (f32: im2col_kernel<float> at k = 4 and 3; bf16: im2col4_bf16_kernel at k = 4 without pad columns, im2col_kernel<bf16> at k = 3
    and at k = 4 with pad columns) and col2im_relu, both types: copies and integer sums, bit-equal, pad columns zero, the sign of a zero kept"""
    first = isinstance(batch, tuple)
    KH, S, P = R.KINDS[kind]
    H, W = hw
    T = BF16 if dt else torch.float32
    g0 = torch.Generator().manual_seed(31 * Ci + 7 * H + W + kind)
    if first:
        xc = [_neg_zeros(_ints(g0, (batch[1], Ci, H, W), -3, 3), g0) for _ in range(batch[0])]
        B = batch[0] * batch[1]
    else:
        xc, B = _neg_zeros(_ints(g0, (batch, H, W, Ci), -3, 3), g0).to(T), batch
    x = [t.to(dev) for t in xc] if first else xc.to(dev)
    OH, OW = R.out_size(H, W, KH, S, P)
    K = Ci * KH * KH
    g = _guard()
    for Kpad in sorted({K, (K + 7) // 8 * 8, K + 8}):        # exact width (the stem's own when K % 8 == 0), the stem's pad8, and a pad of 8
        col = run_im2col(g, dev, dt, x, KH, S, P, Kpad)
        want = R.im2col(xc, KH, S, P, Kpad)
        check_equal(f"im2col Kpad={Kpad}", col, want)
        assert torch.equal(torch.signbit(col.cpu().float()), torch.signbit(want)), f"im2col Kpad={Kpad}: the sign of a zero changed"
        dcolc = _ints(g0, (B * OH * OW, Kpad), -3, 3).to(T)
        actc = _neg_zeros(_ints(g0, (B, H, W, Ci), -3, 3), g0).to(T)
        dX = run_col2im(g, dev, dt, dcolc.to(dev), B, Ci, H, W, KH, S, P, actc.to(dev))
        check_equal(f"col2im_relu Kpad={Kpad}", dX, R.col2im_relu(dcolc, B, Ci, H, W, KH, S, P, actc))
    g.check(f"lowering Ci {Ci} kind {kind} {H} x {W}")


@pytest.mark.parametrize("dt", [0, 1], ids=["f32", "bf16"])
def test_col2im_relu_general(dev, dt):
    """N(0,1) column gradients (bf16-representable): at most k k terms per element, inside the summation bound"""
    T = BF16 if dt else torch.float32
    for Ci, kind, hw in ((16, 0, (20, 36)), (48, 1, (10, 18))):
        KH, S, P = R.KINDS[kind]
        H, W = hw
        OH, OW = R.out_size(H, W, KH, S, P)
        g0 = torch.Generator().manual_seed(Ci + kind)
        dcol = torch.randn(3 * OH * OW, Ci * KH * KH, generator=g0).to(BF16).to(T)
        act = torch.randn(3, H, W, Ci, generator=g0).to(T)
        g = _guard()
        dX = run_col2im(g, dev, dt, dcol.to(dev), 3, Ci, H, W, KH, S, P, act.to(dev))
        g.check("col2im_relu")
        check_bound("col2im_relu " + ("bf16" if dt else "f32"), f"Ci={Ci} k{KH}", dX, *R.col2im_relu(dcol, 3, Ci, H, W, KH, S, P, act, stats=True))


# ---------------------------------------------------------------------------------------------------------------------------------
# the stem, bit-exact across its three paths
@pytest.mark.parametrize("case", R.EXACT_STEMS, ids=lambda c: f"dim{c[0]}-{'tactile' if c[4] else 'image'}-{c[2]}x{c[3]}")
def test_stem_exact_three_paths(dev, case):
    """EarlyCNN.run + backward on a stem whose whole chain is exact in bf16 (conv_refs.exact_stem_case; conditions asserted by
    test_conv_refs_cpu.py): fp32, bf16 on the im2col path and bf16 on the direct path must all give the float64 tokens and all eight
    gradients bit for bit — the wiring of both branches (which activation masks which gradient, the dpreA / dpreB swap, Bsrc against Btot)
    at a tolerance of zero, on rectangular inputs, with 1-3 sources.  At dim 192 both bf16 runs take the im2col path."""
    from m3l_amd.pretrain_models import EarlyCNN
    dim, Cin, H, W, tactile, nsrc, B, seed = case
    xs, params, cot = R.exact_stem_case(*case)
    ref = R.stem(xs, params, tactile, cot)
    stem = EarlyCNN(Cin, dim, key="tactile" if tactile else "image").to(dev)
    with torch.no_grad():
        for p, v in zip(stem._tensors(), params):
            p.copy_(v.to(dev))
    xd, cotd = [x.to(dev) for x in xs], cot.to(dev)
    for dt, direct in (("fp32", 1), ("bf16", 0), ("bf16", 1)):
        old = L.lib().m3l_set_direct_conv(direct)
        try:
            stem.zero_grad(set_to_none=True)
            out = stem.run(xd, dt)
            (out * cotd).sum().backward()
            torch.cuda.synchronize()
        finally:
            L.lib().m3l_set_direct_conv(old)
        what = f"{dt} direct={direct}"
        check_equal(f"{what} tokens", out, ref["tokens"])
        for i, p in enumerate(stem._tensors()):
            check_equal(f"{what} grad {i}", p.grad, ref["grads"][i])
