"""float64 restatement of the EarlyCNN stem's convolution kernels, one function per kernel.  *** TEST INFRASTRUCTURE ONLY ***

The kernels are those of m3l_amd/csrc/conv.hip (conv_fwd_kernel, conv_wgrad_kernel, conv_dgrad_kernel, conv_prep_kernel) and the lowering
kernels of m3l_amd/csrc/elementwise.hip (im2col_kernel, im2col4_bf16_kernel, col2im_relu_kernel), reached through the m3l_op_conv_* /
m3l_op_im2col / m3l_op_col2im_relu exports of include/m3l_amd.h.  One layer is Conv2d(Ci, Co, k, stride s, padding p) + ReLU
(reference models/pretrain_models.py:37-56).

Everything here is index arithmetic on CPU tensors in float64: a loop over the k x k taps, each tap a strided slice of the zero-padded
input.  No call to torch.nn.functional.conv2d / unfold: tests/test_conv_refs_cpu.py anchors these functions against those (1e-12).

An input `x` is either a list of NCHW tensors (the sources of a first layer, concatenated on batch) or one NHWC tensor (an activation).
Outputs are NHWC like the kernels'.  `rnd` (default: identity) is applied where the bf16 kernels store or read a tensor in bf16; with
rnd = bf16_rnd a function is the emulated-bf16 reference.  With stats=True a function also returns, per output element, sum|terms| of
the sum that forms it and the number n of its terms that are not structurally zero (taps inside the image; + 1 for a bias).
"""
import torch

F64 = torch.float64
KINDS = {0: (4, 2, 1), 1: (3, 1, 1)}        # the two layer kinds of the stems: (k, stride, padding)


def ident(t):
    return t


def bf16_rnd(t):
    """round-to-nearest-even to bfloat16, back in float64.  The exact cases feed it integers below 2^24: float64 -> float32 is exact there
    and float32 -> bf16 is the one rounding the kernels make."""
    return t.to(torch.float32).to(torch.bfloat16).to(F64)


def out_size(H, W, KH, S, P):
    return (H + 2 * P - KH) // S + 1, (W + 2 * P - KH) // S + 1


def as_nchw(x):
    """list of NCHW sources | one NHWC activation -> [B, Ci, H, W] float64"""
    if isinstance(x, (list, tuple)):
        return torch.cat([t.to(F64) for t in x], 0)
    return x.to(F64).permute(0, 3, 1, 2).contiguous()


def _padded(xn, P):
    B, C, H, W = xn.shape
    xp = torch.zeros(B, C, H + 2 * P, W + 2 * P, dtype=xn.dtype)
    xp[:, :, P:P + H, P:P + W] = xn
    return xp


def _tap(xp, kh, kw, S, OH, OW):
    """input values under tap (kh, kw) of every output pixel: [B, Ci, OH, OW]"""
    return xp[:, :, kh:kh + S * (OH - 1) + 1:S, kw:kw + S * (OW - 1) + 1:S]


# ---------------------------------------------------------------------------------------------------------------------------------
def conv_fwd(x, w, bias, KH, S, P, rnd=ident, relu=True, stats=False):
    """out[b, oh, ow, co] = relu(bias[co] + sum_(ci, kh, kw) x[b, ci, oh S - P + kh, ow S - P + kw] w[co, ci, kh, kw]), NHWC, rounded once"""
    xn, w = rnd(as_nchw(x)), rnd(w.to(F64))
    B, Ci, H, W = xn.shape
    Co = w.shape[0]
    OH, OW = out_size(H, W, KH, S, P)
    xp, ones = _padded(xn, P), _padded(torch.ones(1, 1, H, W, dtype=F64), P)
    acc = bias.to(F64).view(1, 1, 1, Co).expand(B, OH, OW, Co).clone()
    mag = acc.abs()
    n = torch.ones(OH, OW, dtype=F64)
    for kh in range(KH):
        for kw in range(KH):
            t = _tap(xp, kh, kw, S, OH, OW)
            acc += torch.einsum("bchw,oc->bhwo", t, w[:, :, kh, kw])
            if stats:
                mag += torch.einsum("bchw,oc->bhwo", t.abs(), w[:, :, kh, kw].abs())
                n += Ci * _tap(ones, kh, kw, S, OH, OW)[0, 0]
    out = rnd(torch.relu(acc) if relu else acc)
    if stats:
        return out, mag, n.view(1, OH, OW, 1).expand(B, OH, OW, Co)
    return out


def conv_wgrad(x, dY, KH, S, P, rnd=ident, stats=False):
    """dW[co, ci, kh, kw] = sum_(b, oh, ow) dY[b, oh, ow, co] x[b, ci, oh S - P + kh, ow S - P + kw]; dY NHWC [B, OH, OW, Co]"""
    xn, dY = rnd(as_nchw(x)), rnd(dY.to(F64))
    B, Ci, H, W = xn.shape
    OH, OW = out_size(H, W, KH, S, P)
    assert dY.shape[:3] == (B, OH, OW)
    Co = dY.shape[3]
    xp, ones = _padded(xn, P), _padded(torch.ones(1, 1, H, W, dtype=F64), P)
    dW = torch.zeros(Co, Ci, KH, KH, dtype=F64)
    mag, n = torch.zeros_like(dW), torch.zeros_like(dW)
    for kh in range(KH):
        for kw in range(KH):
            t = _tap(xp, kh, kw, S, OH, OW)
            dW[:, :, kh, kw] = torch.einsum("bhwo,bchw->oc", dY, t)
            if stats:
                mag[:, :, kh, kw] = torch.einsum("bhwo,bchw->oc", dY.abs(), t.abs())
                n[:, :, kh, kw] = B * float(_tap(ones, kh, kw, S, OH, OW).sum())
    return (dW, mag, n) if stats else dW


def conv_dgrad(dY, w, act, KH, S, P, rnd=ident, stats=False):
    """dX[b, ih, iw, ci] = [act > 0] sum over the taps with (ih + P - kh) % S == 0, (iw + P - kw) % S == 0 and the output pixel inside the
    output of sum_co dY[b, (ih + P - kh) / S, (iw + P - kw) / S, co] w[co, ci, kh, kw]; act NHWC [B, H, W, Ci], rounded once"""
    dY, w, act = rnd(dY.to(F64)), rnd(w.to(F64)), act.to(F64)
    B, H, W, Ci = act.shape
    OH, OW = out_size(H, W, KH, S, P)
    assert dY.shape[:3] == (B, OH, OW)
    Co = dY.shape[3]
    acc = torch.zeros(B, Ci, H + 2 * P, W + 2 * P, dtype=F64)
    mag, n = torch.zeros_like(acc), torch.zeros(H + 2 * P, W + 2 * P, dtype=F64)
    for kh in range(KH):
        for kw in range(KH):
            sl = (slice(None), slice(None), slice(kh, kh + S * (OH - 1) + 1, S), slice(kw, kw + S * (OW - 1) + 1, S))
            acc[sl] += torch.einsum("bhwo,oc->bchw", dY, w[:, :, kh, kw])
            if stats:
                mag[sl] += torch.einsum("bhwo,oc->bchw", dY.abs(), w[:, :, kh, kw].abs())
                n[sl[2:]] += Co
    crop = lambda t: t[..., P:P + H, P:P + W]      # noqa: E731
    mask = (act > 0).to(F64)
    dX = rnd(crop(acc).permute(0, 2, 3, 1) * mask)
    if stats:
        return dX, crop(mag).permute(0, 2, 3, 1) * mask, crop(n).view(1, H, W, 1).expand(B, H, W, Ci)
    return dX


# ---------------------------------------------------------------------------------------------------------------------------------
def im2col(x, KH, S, P, Kpad):
    """col[(b OH + oh) OW + ow, (ci k + kh) k + kw] = x[b, ci, oh S - P + kh, ow S - P + kw] (0 outside the image and in the pad columns):
    copies only — the sign of a zero survives"""
    xn = as_nchw(x)
    B, Ci, H, W = xn.shape
    OH, OW = out_size(H, W, KH, S, P)
    assert Kpad >= Ci * KH * KH
    xp = _padded(xn, P)
    col = torch.zeros(B, OH, OW, Kpad, dtype=F64)
    for kh in range(KH):
        for kw in range(KH):
            col[..., kh * KH + kw:Ci * KH * KH:KH * KH] = _tap(xp, kh, kw, S, OH, OW).permute(0, 2, 3, 1)
    return col.reshape(B * OH * OW, Kpad)


def col2im_relu(dcol, B, Ci, H, W, KH, S, P, act, rnd=ident, stats=False):
    """dX[b, ih, iw, ci] = [act > 0] sum over the taps that reach (ih, iw) of dcol[(b, oh, ow), (ci k + kh) k + kw]: the adjoint of im2col"""
    OH, OW = out_size(H, W, KH, S, P)
    Kpad = dcol.shape[1]
    d = dcol.to(F64).reshape(B, OH, OW, Kpad)
    acc = torch.zeros(B, Ci, H + 2 * P, W + 2 * P, dtype=F64)
    mag, n = torch.zeros_like(acc), torch.zeros(H + 2 * P, W + 2 * P, dtype=F64)
    for kh in range(KH):
        for kw in range(KH):
            sl = (slice(None), slice(None), slice(kh, kh + S * (OH - 1) + 1, S), slice(kw, kw + S * (OW - 1) + 1, S))
            t = d[..., kh * KH + kw:Ci * KH * KH:KH * KH].permute(0, 3, 1, 2)
            acc[sl] += t
            mag[sl] += t.abs()
            n[sl[2:]] += 1
    crop = lambda t: t[..., P:P + H, P:P + W]      # noqa: E731
    mask = (act.to(F64) > 0).to(F64)
    dX = rnd(crop(acc).permute(0, 2, 3, 1) * mask)
    if stats:
        return dX, crop(mag).permute(0, 2, 3, 1) * mask, crop(n).view(1, H, W, 1).expand(B, H, W, Ci)
    return dX


# ---------------------------------------------------------------------------------------------------------------------------------
# the weight copies of conv_prep_kernel and the host-side rules of conv.hip, restated
def pad16(x):
    return (x + 15) // 16 * 16


def pad32(x):
    return (x + 31) // 32 * 32


def mt_of(Co):
    return 1 if Co <= 16 else 2 if Co <= 32 else 4 if Co <= 64 else 8


def kind_of(KH, S, P):
    return 0 if (KH, S, P) == (4, 2, 1) else 1 if (KH, S, P) == (3, 1, 1) else -1


def supported(Ci, Co, KH, S, P, first_layer):
    """m3l_conv_direct_supported for bf16, as conv.hip states it"""
    if kind_of(KH, S, P) < 0 or Co % 8 or Co < 8 or Co > 128 or Ci < 1 or Ci > 64:
        return 0
    if not first_layer and Ci % 8:
        return 0
    return int((mt_of(Co), pad16(Ci) // 16) in ((1, 1), (2, 1), (4, 2), (8, 4)))


def wgrad_groups(B, Ci, H, W, Co, KH, S, P):
    OH, OW = out_size(H, W, KH, S, P)
    total = B * ((OH + 7) // 8) * ((OW + 7) // 8)
    return max(1, min(total, max(128, (16 << 20) // (Co * Ci * KH * KH))))


def wgrad_split(B, Ci, H, W, Co, KH, S, P):
    """(tiles, groups, tiles_per_wg, workgroups) of a weight-gradient launch"""
    OH, OW = out_size(H, W, KH, S, P)
    total = B * ((OH + 7) // 8) * ((OW + 7) // 8)
    G = wgrad_groups(B, Ci, H, W, Co, KH, S, P)
    tpw = -(-total // G)
    return total, G, tpw, -(-total // tpw)


def sizes(B, Ci, H, W, Co, KH, S, P):
    """(wf_bytes, wd_bytes, slab_bytes) by the formulas of include/m3l_amd.h"""
    classes, tpc = (4, 4) if S == 2 else (1, KH * KH)
    return (2 * 16 * mt_of(Co) * pad32(KH * KH * pad16(Ci)), 2 * classes * pad16(Ci) * tpc * Co,
            4 * wgrad_groups(B, Ci, H, W, Co, KH, S, P) * Co * Ci * KH * KH)


def wf_layout(w, KH):
    """Wf [16 MT][Kp]: column (kh k + kw) Cip + ci holds w[co, ci, kh, kw]; zero rows co >= Co, zero columns ci >= Ci and past k k Cip"""
    Co, Ci = w.shape[:2]
    Cip = pad16(Ci)
    Wf = torch.zeros(16 * mt_of(Co), pad32(KH * KH * Cip), dtype=F64)
    for kh in range(KH):
        for kw in range(KH):
            c0 = (kh * KH + kw) * Cip
            Wf[:Co, c0:c0 + Ci] = w[:, :, kh, kw].to(F64)
    return Wf


def wd_layout(w, KH, S):
    """Wd [class][Cip][tpc Co]: column t Co + co holds w[co, ci, kh, kw] of the class's t-th tap; rows ci >= Ci zero.
    S == 2 (4x4, pad 1): class 2 a + c = input parity (ih & 1, iw & 1), tap t = 2 dh + dw is (kh, kw) = (1 - a + 2 dh, 1 - c + 2 dw);
    S == 1 (3x3, pad 1): one class, t = kh 3 + kw"""
    Co, Ci = w.shape[:2]
    Cip = pad16(Ci)
    classes, tpc = (4, 4) if S == 2 else (1, KH * KH)
    Wd = torch.zeros(classes, Cip, tpc * Co, dtype=F64)
    for cls in range(classes):
        for t in range(tpc):
            if S == 2:
                kh, kw = 1 - (cls >> 1) + 2 * (t >> 1), 1 - (cls & 1) + 2 * (t & 1)
            else:
                kh, kw = t // 3, t % 3
            Wd[cls, :Ci, t * Co:(t + 1) * Co] = w[:, :, kh, kw].to(F64).t()
    return Wd


# ---------------------------------------------------------------------------------------------------------------------------------
def stem_kinds(tactile):
    return [KINDS[0], KINDS[0], KINDS[1] if tactile else KINDS[0]]


def stem(xs, params, tactile, cot=None, rnd=ident):
    """The four-layer stem and its backward, composed from the functions above the way m3l_earlycnn_fwd / _bwd wire them.
    xs: list of NCHW sources; params: [w1, b1, ..., w4, b4] (w4 [D, D/2, 1, 1]); cot: cotangent of the tokens [B, h w, D].
    Returns a dict: tokens (f32 in the library: not rounded), act (the three NHWC activations, stored in the compute type), and with cot:
    dout (cot in the compute type), dpre (the gradients at the three pre-activations, index = layer, stored in the compute type) and
    grads (the eight parameter gradients)."""
    p = [t.to(F64) for t in params]
    kinds = stem_kinds(tactile)
    act, x = [], list(xs)
    for l in range(3):
        KH, S, P = kinds[l]
        x = conv_fwd(x, p[2 * l], p[2 * l + 1], KH, S, P, rnd=rnd)
        act.append(x)
    B, h, w_, C3 = x.shape
    w4 = rnd(p[6].reshape(p[6].shape[0], C3))
    tokens = (x.reshape(B, h * w_, C3) @ w4.t()) + p[7]
    r = dict(tokens=tokens, act=act)
    if cot is None:
        return r
    cot = cot.to(F64)
    dout = rnd(cot)
    grads = [None] * 8
    a3 = x.reshape(B * h * w_, C3)
    d2 = dout.reshape(B * h * w_, -1)
    grads[6] = (d2.t() @ a3).reshape(p[6].shape)
    grads[7] = cot.reshape(B * h * w_, -1).sum(0)            # the bias gradient sums the f32 cotangent, not its rounded copy
    dpre = [None] * 3
    dpre[2] = rnd((d2 @ w4) * (a3 > 0).to(F64)).reshape(B, h, w_, C3)
    for l in (2, 1, 0):
        KH, S, P = kinds[l]
        src = list(xs) if l == 0 else act[l - 1]
        grads[2 * l] = conv_wgrad(src, dpre[l], KH, S, P, rnd=rnd)
        grads[2 * l + 1] = dpre[l].sum((0, 1, 2))
        if l:
            dpre[l - 1] = conv_dgrad(dpre[l], p[2 * l], act[l - 1], KH, S, P, rnd=rnd)
    r.update(dout=dout, dpre=dpre, grads=grads)
    return r


def exact_stem_case(dim, C, H, W, tactile, nsrc, B, seed):
    """An EarlyCNN whose whole chain is exact in bf16 (section "stem-level" of tests/test_conv_kernels_gpu.py): inputs in {0, 1, 2}, every
    conv weight with at most two non-zero entries (+-1) per output channel at seeded positions, biases in {0, 1, 2}, cotangents integers in
    [-2, 2].  Returns (xs, params, cot), float32 CPU tensors."""
    g = torch.Generator().manual_seed(seed)
    co = [dim // 8, dim // 4, dim // 2, dim]
    ks = [4, 4, 3 if tactile else 4, 1]
    xs = [torch.randint(0, 3, (B, C, H, W), generator=g).float() for _ in range(nsrc)]
    params, ci = [], C
    for l in range(4):
        w = torch.zeros(co[l], ci * ks[l] * ks[l])
        pos = torch.randint(0, w.shape[1], (co[l], 2), generator=g)
        sgn = torch.randint(0, 2, (co[l], 2), generator=g).float() * 2 - 1
        w[torch.arange(co[l]), pos[:, 0]] = sgn[:, 0]
        w[torch.arange(co[l]), pos[:, 1]] = sgn[:, 1]        # the same position twice: one non-zero entry
        params += [w.reshape(co[l], ci, ks[l], ks[l]), torch.randint(0, 3, (co[l],), generator=g).float()]
        ci = co[l]
    h, w_ = H, W
    for l in range(3):
        h, w_ = out_size(h, w_, *stem_kinds(tactile)[l])
    cot = torch.randint(-2, 3, (nsrc * B, h * w_, dim), generator=g).float()
    return xs, params, cot


# (dim, C, H, W, tactile, nsrc, B, seed): the pinned cases; test_conv_refs_cpu.py asserts that every value the library stores in bf16 is an
# integer of magnitude <= 256 in the reference and that at least a quarter of each layer's activations are non-zero
EXACT_STEMS = [
    (64, 3, 16, 24, False, 1, 2, 0),
    (192, 12, 24, 40, False, 1, 1, 0),
    (192, 3, 12, 20, True, 2, 1, 0),
    (256, 12, 8, 16, True, 3, 1, 0),
]
