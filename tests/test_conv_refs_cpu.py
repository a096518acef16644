"""CPU checks behind tests/test_conv_kernels_gpu.py: the float64 restatement of tests/conv_refs.py against torch's own conv2d / unfold with
autograd in float64 (1e-12 relative), the m3l_op_conv_* exports' sizes, refusals and support rule (nothing is launched: every call here is
refused before its launch or is host-only), and the conditions that make the pinned stem cases exact in bf16."""
import ctypes as C
import os

import pytest
import torch
import torch.nn.functional as F

import conv_refs as R
from m3l_amd import _lib as L

F64 = torch.float64
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
S2_GEOS = [(16, 16), (20, 36), (36, 20), (6, 34), (2, 4), (34, 18)]
K3_GEOS = [(8, 8), (10, 18), (18, 10), (3, 6), (1, 2)]
CASES = [(kind, hw) for kind, geos in ((0, S2_GEOS), (1, K3_GEOS)) for hw in geos]


def _close(a, b, what):
    assert a.shape == b.shape, (what, a.shape, b.shape)
    err = float((a - b).abs().max()) if a.numel() else 0.0
    assert err <= 1e-12 * max(1.0, float(b.abs().max())), f"{what}: {err}"


def _data(kind, hw, Ci, Co, nchw, seed):
    KH, S, P = R.KINDS[kind]
    H, W = hw
    g = torch.Generator().manual_seed(seed)
    if nchw:
        x = [torch.randn(b, Ci, H, W, generator=g, dtype=F64) for b in (2, 1)]
        xn = torch.cat(x, 0)
    else:
        x = torch.randn(3, H, W, Ci, generator=g, dtype=F64)
        xn = x.permute(0, 3, 1, 2).contiguous()
    OH, OW = R.out_size(H, W, KH, S, P)
    w = torch.randn(Co, Ci, KH, KH, generator=g, dtype=F64)
    b = torch.randn(Co, generator=g, dtype=F64)
    dY = torch.randn(3, OH, OW, Co, generator=g, dtype=F64)
    return x, xn, w, b, dY, (KH, S, P, H, W, OH, OW)


@pytest.mark.parametrize("kind,hw", CASES)
@pytest.mark.parametrize("Ci,Co,nchw", [(3, 8, 1), (24, 16, 0)])
def test_conv_restatement_matches_torch_float64(kind, hw, Ci, Co, nchw):
    x, xn, w, b, dY, (KH, S, P, H, W, OH, OW) = _data(kind, hw, Ci, Co, nchw, 7 * hw[0] + hw[1] + Ci)
    xa, wa, ba = xn.clone().requires_grad_(True), w.clone().requires_grad_(True), b.clone().requires_grad_(True)
    pre = F.conv2d(xa, wa, ba, stride=S, padding=P)
    assert pre.shape[2:] == (OH, OW)
    out, mag, n = R.conv_fwd(x, w, b, KH, S, P, stats=True)
    _close(out, torch.relu(pre).permute(0, 2, 3, 1).detach(), "forward")
    _close(R.conv_fwd(x, w, b, KH, S, P), out, "forward without stats")
    _close(mag, F.conv2d(xn.abs(), w.abs(), b.abs(), stride=S, padding=P).permute(0, 2, 3, 1), "forward sum|terms|")
    _close(n, (F.conv2d(torch.ones_like(xn), torch.ones_like(w), None, stride=S, padding=P) + 1).permute(0, 2, 3, 1), "forward n")
    # gradients of the convolution alone (the ReLU of THIS layer is the caller's): cotangent dY at the pre-activation
    gx, gw = torch.autograd.grad((pre * dY.permute(0, 3, 1, 2)).sum(), (xa, wa))
    dW, wmag, wn = R.conv_wgrad(x, dY, KH, S, P, stats=True)
    _close(dW, gw, "weight gradient")
    act = torch.randn(3, H, W, Ci, generator=torch.Generator().manual_seed(H), dtype=F64)
    act[0, 0, 0, 0], act[0, 0, -1, -1] = 0.0, -0.0
    dX, xmag, xnn = R.conv_dgrad(dY, w, act, KH, S, P, stats=True)
    mask = (act > 0).to(F64)
    _close(dX, gx.permute(0, 2, 3, 1) * mask, "input gradient")
    ga, = torch.autograd.grad(F.conv2d(xa, wa.detach().abs(), None, stride=S, padding=P), xa, dY.permute(0, 3, 1, 2).abs())
    _close(xmag, ga.permute(0, 2, 3, 1) * mask, "input gradient sum|terms|")
    xo = torch.ones_like(xn).requires_grad_(True)
    go, = torch.autograd.grad(F.conv2d(xo, torch.ones_like(w), None, stride=S, padding=P).sum(), xo)
    _close(xnn, go.permute(0, 2, 3, 1), "input gradient n")
    gwa, = torch.autograd.grad(F.conv2d(xn.abs(), wa, None, stride=S, padding=P), wa, dY.permute(0, 3, 1, 2).abs())
    _close(wmag, gwa, "weight gradient sum|terms|")
    gwo, = torch.autograd.grad(F.conv2d(torch.ones_like(xn), wa, None, stride=S, padding=P).sum(), wa)
    _close(wn, gwo.expand_as(wn), "weight gradient n")


@pytest.mark.parametrize("kind,hw", CASES)
@pytest.mark.parametrize("Ci,nchw,extra", [(3, 1, 5), (8, 0, 0)])
def test_column_matrix_and_adjoint_match_unfold(kind, hw, Ci, nchw, extra):
    x, xn, w, b, dY, (KH, S, P, H, W, OH, OW) = _data(kind, hw, Ci, 8, nchw, 3 * hw[0] + hw[1])
    K = Ci * KH * KH
    Kpad = K + extra
    col = R.im2col(x, KH, S, P, Kpad)
    ref = F.unfold(xn, KH, padding=P, stride=S).transpose(1, 2).reshape(3 * OH * OW, K)
    assert torch.equal(col[:, :K], ref) and not col[:, K:].any()
    g = torch.Generator().manual_seed(W)
    dcol = torch.randn(3 * OH * OW, Kpad, generator=g, dtype=F64)
    act = torch.randn(3, H, W, Ci, generator=g, dtype=F64)
    dX, mag, n = R.col2im_relu(dcol, 3, Ci, H, W, KH, S, P, act, stats=True)
    fold = lambda t: F.fold(t[:, :K].reshape(3, OH * OW, K).transpose(1, 2), (H, W), KH, padding=P, stride=S).permute(0, 2, 3, 1)  # noqa: E731
    mask = (act > 0).to(F64)
    _close(dX, fold(dcol) * mask, "col2im_relu")
    _close(mag, fold(dcol.abs()) * mask, "col2im_relu sum|terms|")
    _close(n, fold(torch.ones_like(dcol)), "col2im_relu n")
    # the column matrix times the flattened weight is the convolution: ties the K order to the Conv2d weight layout
    _close((col[:, :K] @ w.reshape(8, K).t() + b).reshape(3, OH, OW, 8), F.conv2d(xn, w, b, stride=S, padding=P).permute(0, 2, 3, 1), "col W^T")


@pytest.mark.parametrize("Ci,Co,kind", [(3, 8, 0), (24, 48, 0), (48, 96, 1), (12, 24, 0)])
def test_weight_layouts_reproduce_the_convolution(Ci, Co, kind):
    """Wf / Wd as conv_refs restates them, used the way the kernels use them, give the convolution and its input gradient"""
    KH, S, P = R.KINDS[kind]
    g = torch.Generator().manual_seed(Ci + Co)
    w = torch.randn(Co, Ci, KH, KH, generator=g, dtype=F64)
    Cip = R.pad16(Ci)
    Wf = R.wf_layout(w, KH)
    assert Wf.shape == (16 * R.mt_of(Co), R.pad32(KH * KH * Cip)) and Wf.numel() * 2 == R.sizes(1, Ci, 8, 8, Co, KH, S, P)[0]
    back = Wf[:Co, :KH * KH * Cip].reshape(Co, KH, KH, Cip)
    assert torch.equal(back[..., :Ci].permute(0, 3, 1, 2), w) and not back[..., Ci:].any() and not Wf[Co:].any() and not Wf[:, KH * KH * Cip:].any()
    Wd = R.wd_layout(w, KH, S)
    assert Wd.numel() * 2 == R.sizes(1, Ci, 8, 8, Co, KH, S, P)[1] and not Wd[:, Ci:].any()
    H, W = (6, 10) if S == 2 else (5, 7)
    OH, OW = R.out_size(H, W, KH, S, P)
    dY = torch.randn(1, OH, OW, Co, generator=g, dtype=F64)
    want = R.conv_dgrad(dY, w, torch.ones(1, H, W, Ci, dtype=F64), KH, S, P)
    dYp = torch.zeros(OH + 2, OW + 2, Co, dtype=F64)
    dYp[1:-1, 1:-1] = dY[0]
    got = torch.zeros(H, W, Ci, dtype=F64)
    for ih in range(H):
        for iw in range(W):
            a, c = (ih & 1, iw & 1) if S == 2 else (0, 0)
            taps = []
            for t in range(Wd.shape[2] // Co):
                if S == 2:      # conv_dgrad_kernel: oh = (ih >> 1) + a - dh, ow = (iw >> 1) + c - dw
                    taps.append(dYp[(ih >> 1) + a - (t >> 1) + 1, (iw >> 1) + c - (t & 1) + 1])
                else:           # oh = ih + 1 - kh
                    taps.append(dYp[ih + 1 - t // 3 + 1, iw + 1 - t % 3 + 1])
            got[ih, iw] = (Wd[2 * a + c] @ torch.cat(taps))[:Ci]
    _close(got, want[0], "Wd applied per parity class")


@pytest.mark.parametrize("case", R.EXACT_STEMS)
def test_stem_restatement_and_exact_cases(case):
    """the composed stem against torch autograd in float64, on the pinned exact cases; and the two conditions that make those cases a
    bit-exact test of the bf16 library: every bf16-stored value is an integer of magnitude <= 256, at least a quarter of each layer's
    activations are non-zero"""
    dim, Cin, H, W, tactile, nsrc, B, seed = case
    xs, params, cot = R.exact_stem_case(*case)
    for l in range(4):
        assert int((params[2 * l].flatten(1) != 0).sum(1).max()) <= 2 and set(params[2 * l].unique().tolist()) <= {-1.0, 0.0, 1.0}
    r = R.stem(xs, params, tactile, cot)
    rb = R.stem(xs, params, tactile, cot, rnd=R.bf16_rnd)
    pa = [p.to(F64).requires_grad_(True) for p in params]
    h = torch.cat([x.to(F64) for x in xs], 0)
    kinds = R.stem_kinds(tactile)
    acts = []
    for l in range(3):
        h = torch.relu(F.conv2d(h, pa[2 * l], pa[2 * l + 1], stride=kinds[l][1], padding=kinds[l][2]))
        h.retain_grad()
        acts.append(h)
    tok = F.conv2d(h, pa[6], pa[7]).flatten(2).transpose(1, 2)
    (tok * cot.to(F64)).sum().backward()
    _close(r["tokens"], tok.detach(), "tokens")
    for l in range(3):
        _close(r["act"][l], acts[l].detach().permute(0, 2, 3, 1), f"act{l}")
        _close(r["dpre"][l], (acts[l].grad * (acts[l] > 0)).permute(0, 2, 3, 1), f"dpre{l}")
    for i in range(8):
        _close(r["grads"][i], pa[i].grad, f"grad{i}")
    stored = r["act"] + r["dpre"] + [r["dout"]]
    for t in stored:
        assert torch.equal(t, t.round()) and float(t.abs().max()) <= 256
    for l in range(3):
        assert float((r["act"][l] != 0).double().mean()) >= 0.25, (l, float((r["act"][l] != 0).double().mean()))
    # hence the emulated-bf16 stem is the exact stem, and every result is an integer below 2^24: any f32 summation order is exact
    for k in ("tokens", "dout"):
        assert torch.equal(r[k], rb[k])
    for a, b in zip(r["act"] + r["dpre"] + r["grads"], rb["act"] + rb["dpre"] + rb["grads"]):
        assert torch.equal(a, b) and torch.equal(a, a.round()) and float(a.abs().max()) < 2 ** 24
    mags = R.stem([x.abs() for x in xs], [p.abs() for p in params], tactile, cot.abs())     # every sum's sum|terms| stays below 2^24 too
    assert max(float(t.abs().max()) for t in mags["grads"] + [mags["tokens"]]) < 2 ** 24


# ---------------------------------------------------------------------------------------------------------------------------------
# the exports, without a launch
def test_version_and_header():
    assert L.lib().m3l_version() >= 416
    hdr = open(os.path.join(ROOT, "include", "m3l_amd.h")).read()
    assert "(ABI 416)" in hdr and "as im2col + MFMA GEMM.  srcs" not in hdr
    for name in ("supported", "sizes", "prep", "fwd", "wgrad", "dgrad"):
        assert f"m3l_op_conv_{name}(" in hdr


def _sizes(*a):
    out = [C.c_size_t(0) for _ in range(3)]
    rc = L.lib().m3l_op_conv_sizes(*a, *[C.byref(o) for o in out])
    return rc, tuple(o.value for o in out)


@pytest.mark.parametrize("Ci,Co", [(3, 8), (8, 16), (16, 32), (6, 16), (32, 64), (12, 24), (24, 48), (48, 96), (12, 32), (64, 128)])
def test_sizes_follow_the_header_formulas(Ci, Co):
    for kind, geos in ((0, S2_GEOS + [(16, 48)]), (1, K3_GEOS)):
        KH, S, P = R.KINDS[kind]
        for H, W in geos:
            for B in (1, 3, 43, 2731):
                rc, got = _sizes(B, Ci, H, W, Co, KH, S, P)
                assert rc == 0 and got == R.sizes(B, Ci, H, W, Co, KH, S, P), (B, Ci, H, W, Co, kind, got)
    assert L.lib().m3l_op_conv_sizes(3, Ci, 16, 16, Co, 4, 2, 1, None, None, None) == 0          # each pointer is optional
    # the issue's example: (64, 128) at 16 x 48, B = 43: 129 tiles, 128 groups, 2 tiles per workgroup, 65 workgroups
    assert R.wgrad_split(43, 64, 16, 48, 128, 4, 2, 1) == (129, 128, 2, 65)


def test_supported_rule():
    lib = L.lib()
    for KH, S, P in ((4, 2, 1), (3, 1, 1), (3, 2, 1), (4, 2, 0), (4, 1, 1), (1, 1, 0)):
        for first in (0, 1):
            for Ci in range(1, 137):
                for Co in range(1, 137):
                    assert lib.m3l_op_conv_supported(Ci, Co, KH, S, P, first) == R.supported(Ci, Co, KH, S, P, first), (Ci, Co, KH, S, P, first)
    stems = {64: [(3, 8), (8, 16), (16, 32)], 128: [(6, 16), (16, 32), (32, 64)], 192: [(12, 24), (24, 48), (48, 96)], 256: [(12, 32), (32, 64), (64, 128)]}
    # every layer of the four stems has a direct kernel except the third layer of dim 192: Ci = 48 is three 16-channel tiles and Co = 96 eight,
    # and conv.hip has no (8, 3) weight-gradient template — so the dim-192 stem as a whole keeps the im2col path (cnn_direct, mae_plan.hip)
    for dim, layers in stems.items():
        for l, (Ci, Co) in enumerate(layers):
            want = int((dim, l) != (192, 2))
            assert R.supported(Ci, Co, 4, 2, 1, l == 0) == want and (l < 2 or R.supported(Ci, Co, 3, 1, 1, 0) == want), (dim, l)


FAKE = 0x1000          # a non-null address that a refused call never touches


def _srcs(n, null_at=None):
    arr = (C.c_void_p * max(1, n))()
    for i in range(n):
        arr[i] = None if i == null_at else FAKE
    return arr


def _refused(rc, text):
    assert rc != 0, f"not refused (wanted: {text})"
    assert text in L.last_error(), (text, L.last_error())


def test_refusals_come_with_a_message_and_without_a_launch():
    lib = L.lib()
    ok = (8, 16, 16, 16, 4, 2, 1)                     # Ci, H, W, Co, k, s, p of a supported NHWC layer

    def fwd(srcs=None, nsrc=1, nchw=0, Bsrc=3, shape=ok, Wf=FAKE, bias=FAKE, out=FAKE):
        return lib.m3l_op_conv_fwd(_srcs(nsrc) if srcs is None else srcs, nsrc, nchw, Bsrc, *shape, Wf, bias, out, None)

    def wgrad(srcs=None, nsrc=1, nchw=0, Bsrc=3, shape=ok, dY=FAKE, slab=FAKE, dW=FAKE):
        return lib.m3l_op_conv_wgrad(_srcs(nsrc) if srcs is None else srcs, nsrc, nchw, Bsrc, *shape, dY, slab, dW, None)

    def dgrad(dY=FAKE, B=3, shape=ok, Wd=FAKE, act=FAKE, dX=FAKE):
        return lib.m3l_op_conv_dgrad(dY, B, *shape, Wd, act, dX, None)

    def im2col(dtype=1, srcs=None, nsrc=1, nchw=0, Bsrc=3, shape=(8, 16, 16, 4, 2, 1), Kpad=128, col=FAKE):
        return lib.m3l_op_im2col(dtype, _srcs(nsrc) if srcs is None else srcs, nsrc, nchw, Bsrc, *shape, Kpad, col, None)

    def col2im(dtype=1, dcol=FAKE, B=3, shape=(8, 16, 16, 4, 2, 1), Kpad=128, act=FAKE, dX=FAKE):
        return lib.m3l_op_col2im_relu(dtype, dcol, B, *shape, Kpad, act, dX, None)

    # null pointers
    _refused(lib.m3l_op_conv_fwd(None, 1, 0, 3, *ok, FAKE, FAKE, FAKE, None), "op_conv_fwd: null pointer (srcs)")
    _refused(lib.m3l_op_conv_wgrad(None, 1, 0, 3, *ok, FAKE, FAKE, FAKE, None), "op_conv_wgrad: null pointer (srcs)")
    _refused(lib.m3l_op_im2col(1, None, 1, 0, 3, 8, 16, 16, 4, 2, 1, 128, FAKE, None), "op_im2col: null pointer (srcs)")
    for call, name in ((fwd, "op_conv_fwd"), (wgrad, "op_conv_wgrad"), (im2col, "op_im2col")):
        _refused(call(srcs=_srcs(2, null_at=1), nsrc=2, nchw=1), f"{name}: null pointer (srcs[1])")
    for kw in ("Wf", "bias", "out"):
        _refused(fwd(**{kw: None}), "op_conv_fwd: null pointer")
    for kw in ("dY", "slab", "dW"):
        _refused(wgrad(**{kw: None}), "op_conv_wgrad: null pointer")
    for kw in ("dY", "Wd", "act", "dX"):
        _refused(dgrad(**{kw: None}), "op_conv_dgrad: null pointer")
    _refused(im2col(col=None), "op_im2col: null pointer")
    for kw in ("dcol", "act", "dX"):
        _refused(col2im(**{kw: None}), "op_col2im_relu: null pointer")
    _refused(lib.m3l_op_conv_prep(None, 8, 16, 4, 2, FAKE, FAKE, None), "op_conv_prep: null pointer")
    _refused(lib.m3l_op_conv_prep(FAKE, 8, 16, 4, 2, None, FAKE, None), "op_conv_prep: null pointer")
    # source counts
    for call, name in ((fwd, "op_conv_fwd"), (wgrad, "op_conv_wgrad"), (im2col, "op_im2col")):
        for n in (0, 9, -1):
            _refused(call(srcs=_srcs(9), nsrc=n, nchw=1), f"{name}: nsrc={n} outside 1..8")
        _refused(call(nsrc=2, nchw=0), f"{name}: an NHWC input is one source (nsrc=2)")
    # sizes: output below 1, odd H / W under stride 2, batch below 1
    small, oddh, oddw = (8, 1, 2, 16, 4, 2, 1), (8, 15, 16, 16, 4, 2, 1), (8, 16, 7, 16, 4, 2, 1)
    calls = ((fwd, "op_conv_fwd", {}), (wgrad, "op_conv_wgrad", {}), (dgrad, "op_conv_dgrad", {}), (im2col, "op_im2col", {}), (col2im, "op_col2im_relu", {}))
    for call, name, _ in calls:
        lower = name in ("op_im2col", "op_col2im_relu")
        cut = (lambda s: s[:3] + s[4:]) if lower else (lambda s: s)
        _refused(call(shape=cut(small)), f"{name}: output size below 1")
        _refused(call(shape=cut(oddh)), f"{name}: odd H=15 or W=16 with the 4x4 / stride-2 convolution")
        _refused(call(shape=cut(oddw)), f"{name}: odd H=16 or W=7 with the 4x4 / stride-2 convolution")
        _refused(call(**{"B" if name in ("op_conv_dgrad", "op_col2im_relu") else "Bsrc": 0}), f"{name}: bad sizes B=0")
    rc, _ = _sizes(3, 8, 1, 2, 16, 4, 2, 1)
    _refused(rc, "op_conv_sizes: output size below 1")
    rc, _ = _sizes(3, 8, 16, 16, 16, 5, 2, 1)
    _refused(rc, "op_conv_sizes: k=5 s=2 p=1 is neither 4/2/1 nor 3/1/1")
    # an odd size is fine where the stride is 1, and for a lowering of another kernel size
    assert R.out_size(3, 7, 3, 1, 1) == (3, 7)
    # shapes without a direct kernel: Ci not a multiple of 8 behind the first layer, Co not a multiple of 8, another (MT, NT), another kind
    for shape in ((12, 16, 16, 24, 4, 2, 1), (8, 16, 16, 20, 4, 2, 1), (64, 16, 16, 16, 4, 2, 1), (8, 16, 16, 16, 4, 1, 1), (8, 16, 16, 136, 4, 2, 1)):
        text = f"no direct convolution for Ci={shape[0]} Co={shape[3]} k={shape[4]} s={shape[5]} p={shape[6]} (NHWC bf16 input)"
        _refused(fwd(shape=shape), "op_conv_fwd: " + text)
        _refused(wgrad(shape=shape), "op_conv_wgrad: " + text)
        _refused(dgrad(shape=shape), "op_conv_dgrad: " + text)
    _refused(fwd(nchw=1, shape=(72, 16, 16, 16, 4, 2, 1)), "op_conv_fwd: no direct convolution for Ci=72 Co=16 k=4 s=2 p=1 (NCHW f32 input)")
    _refused(dgrad(shape=(24, 10, 18, 48, 3, 1, 1)), "op_conv_dgrad: taps x Co = 9 x 48 must be a multiple of 32")
    _refused(lib.m3l_op_conv_prep(FAKE, 24, 48, 3, 1, FAKE, FAKE, None), "op_conv_prep: Wd needs taps x Co = 9 x 48 a multiple of 32")
    _refused(lib.m3l_op_conv_prep(FAKE, 12, 24, 4, 2, FAKE, FAKE, None), "op_conv_prep: no direct convolution for Ci=12 Co=24")
    _refused(lib.m3l_op_conv_prep(FAKE, 8, 20, 4, 2, FAKE, None, None), "op_conv_prep: no direct convolution for Ci=8 Co=20")
    # the lowering kernels: dtype and Kpad
    _refused(im2col(dtype=2), "op_im2col: bad dtype 2")
    _refused(col2im(dtype=-1), "op_col2im_relu: bad dtype -1")
    _refused(im2col(Kpad=127), "op_im2col: Kpad=127 below Ci k k = 128")
    _refused(col2im(Kpad=127), "op_col2im_relu: Kpad=127 below Ci k k = 128")
