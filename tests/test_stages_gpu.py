"""The MAE step's stage kernels one by one, through their m3l_amd.functional entry points, against the float64 restatement of
tests/stage_refs.py (anchored by tests/test_stage_refs_cpu.py), in fp32 and bf16 compute.  Needs the MI355X.

Stages: Fn.mask_sample, Fn.EmbedFn, Fn.TokensAssembleFn, Fn.UnshuffleFn, Fn.HeadsLossFn, Fn.GatherTokensFn — each with sink=None and
Fn.make_geom on a small VTT.  Parameters are drawn away from initialisation (LayerNorm gains 1 + 0.5 N(0,1); biases, modality rows and
mask token 0.4 N(0,1); weights 2 / sqrt(K) N(0,1); cotangents N(0,1)).  Inputs are `rand` frames in which every seventh patch is constant
and one whole frame is constant.  The constants are multiples of 1/8: the f32 sum and mean of such a patch are exact, so its variance is
exactly 0 on both sides (rstd = 1 / sqrt(eps) = 316) and its normalised value exactly 0.  A constant that is not dyadic leaves a last-bit
residue in any f32 mean, which that rstd multiplies by 316: a property of LayerNorm in f32 (torch's too), not of these kernels.

Bounds (H = HIP result, X = exact float64 result, R = float64 result with the bf16 storage roundings of stage_refs, u = 2^-24):
  exact   copies and index lists: bit-equal
  sum     outputs that are sums or copies of exact f32 inputs, in BOTH compute types (downstream of no rounding): per element
          |H - X| <= c u sum|terms|, the bound of fixed-order f32 summation; sum|terms| comes from the reference, c is the longest chain of
          additions a term passes through in the kernel, read off the kernel beside each use (`_chain`)
  gemm    every other fp32 output: max|H - X| <= 2e-5 max|X| (the bound of test_gemm_nt_plain / test_gemm_tn in test_kernels_gpu.py)
  bf16    outputs downstream of a rounding: max|H - X| <= 2 max|R - X| + 2e-5 max|X|, and ||H - X|| / ||X|| <= 1.5 ||R - X|| / ||X|| + 2e-5.
          R is independent of the code under test; its distance to X is the noise these roundings must cost.
The measured ratios are printed per check and the worst per stage at the end of the module (recorded in EXPERIMENTS.md).
"""
import functools
import math
import zlib

import pytest
import torch

import stage_refs as R

pytestmark = pytest.mark.gpu

from m3l_amd import _lib as L  # noqa: E402
from m3l_amd import functional as Fn  # noqa: E402
from m3l_amd.pretrain_models import VTT  # noqa: E402

F64 = torch.float64
U = 2.0 ** -24
GEMM_FP32 = 2e-5
DTS = ["fp32", "bf16"]
WORST = {}          # (stage, dt) -> {metric: worst value}


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    L.lib()
    yield torch.device("cuda:0")
    for (stage, dt), m in sorted(WORST.items()):
        print(f"[stages worst] {stage:16s} {dt:5s} " + "  ".join(f"{k}={v:.3g}" for k, v in sorted(m.items())))


# -------------------------------------------------------------------------------------------------------------------
# bounds
def _note(stage, dt, metric, value, what):
    w = WORST.setdefault((stage, dt), {})
    w[metric] = max(w.get(metric, 0.0), float(value))
    print(f"[stages] {stage} {dt} {what}: {metric}={float(value):.3g}")


def _d(t):
    return t.detach().to("cpu", F64)


def check_exact(stage, dt, what, H, X):
    assert H.dtype == X.dtype and torch.equal(H.detach().cpu(), X), f"{stage} {what}: not bit-equal"


def check_sum(stage, dt, what, H, X, terms, c):
    """|H - X| <= c u sum|terms| per element; where the bound is 0 the result is exact"""
    H, X, bound = _d(H), _d(X), c * U * _d(terms)
    err = (H - X).abs()
    frac = float((err / bound.clamp_min(1e-300)).max()) if err.numel() else 0.0
    _note(stage, dt, "sum_frac", frac, f"{what} (c={c})")
    assert frac <= 1.0, f"{stage} {what}: {frac:.3g} of the summation bound (c={c})"


def check_gemm(stage, dt, what, H, X):
    H, X = _d(H), _d(X)
    frac = float((H - X).abs().max()) / (GEMM_FP32 * max(float(X.abs().max()), 1e-300))
    _note(stage, dt, "gemm_frac", frac, what)
    assert frac <= 1.0, f"{stage} {what}: max error {frac:.3g} of 2e-5 max|X|"


def check_bf16(stage, dt, what, H, X, Rr):
    H, X, Rr = _d(H), _d(X), _d(Rr)
    xm, xn = max(float(X.abs().max()), 1e-300), max(float(X.norm()), 1e-300)
    eh, er = float((H - X).abs().max()), float((Rr - X).abs().max())
    lh, lr = float((H - X).norm()) / xn, float((Rr - X).norm()) / xn
    _note(stage, dt, "max_ratio", eh / max(er, 1e-300), what)
    _note(stage, dt, "l2_ratio", lh / max(lr, 1e-300), what)
    assert eh <= 2.0 * er + GEMM_FP32 * xm, f"{stage} {what}: max|H-X| = {eh:.3g}, max|R-X| = {er:.3g}, max|X| = {xm:.3g}"
    assert lh <= 1.5 * lr + GEMM_FP32, f"{stage} {what}: rel L2 H {lh:.3g}, R {lr:.3g}"


def check_val(stage, dt, what, H, X, Rr):
    """an output downstream of a GEMM / a rounding: `gemm` in fp32, `bf16` in bf16"""
    if dt == "bf16":
        check_bf16(stage, dt, what, H, X, Rr)
    else:
        check_gemm(stage, dt, what, H, X)


def _part_grid(rows):
    """elementwise.hip part_grid: one wave per row, WPB = 4 rows per block, at most m3l_part_blocks() = 1024 blocks"""
    return max(1, min((rows + 3) // 4, 1024))


def _reduce_chain(G):
    """reduce_cols_32x32 over G partial rows: a slice adds ceil(G / 256) rows into each of 8 accumulators (+ up to 7 tail rows into the
    first), a 3-level tree joins them, then the 32 slices are added one after the other"""
    return (G + 255) // 256 + 7 + 3 + 31


def _chain(rows):
    """embed_finalize_bwd_kernel / tokens_assemble_bwd_kernel: a wave adds its ceil(rows / 4 G) rows one by one into its LDS slab, the four
    slabs are added in order (3), then the partial rows are reduced"""
    G = _part_grid(rows)
    return (rows + 4 * G - 1) // (4 * G) + 3 + _reduce_chain(G)


# -------------------------------------------------------------------------------------------------------------------
# data
def _gen(name):
    return torch.Generator().manual_seed(zlib.crc32(name.encode()))


def _pair(v):
    return v if isinstance(v, tuple) else (v, v)


def _frames(gen, B, C, hw, P, whole=None):
    """rand frames; every seventh patch constant (a multiple of 1/8), frame `whole` constant 0.5"""
    H, W = _pair(hw)
    x = torch.rand(B, C, H, W, generator=gen)
    gh, gw = H // P, W // P
    for b in range(B):
        for p in range(gh * gw):
            if (b * gh * gw + p) % 7 == 3:
                ph, pw = divmod(p, gw)
                x[b, :, ph * P:(ph + 1) * P, pw * P:(pw + 1) * P] = ((b + p) % 9) / 8.0
    if whole is not None:
        x[whole] = 0.5
    return x


def _geom_of(s, use_vision=True, use_tactile=True):
    """Fn.make_geom on a small VTT of the case's geometry (the VTT's own width plays no part: the stages take D as an argument)"""
    enc = VTT(image_size=_pair(s["img"]), tactile_size=_pair(s["tac"]), image_patch_size=s["Pi"], tactile_patch_size=s["Pt"], dim=64, depth=1,
              heads=1, mlp_dim=64, image_channels=s["Ci"], tactile_channels=s["Ct"], num_tactiles=s["k"])
    return Fn.make_geom(enc, s["k"], use_vision and s.get("vision", True), use_tactile and s.get("tactile", True))


def _inputs(gen, s, B):
    """image, tactiles (None / [] for an absent modality); the last sensor's frame of sample B // 2 is constant (the image's without sensors)"""
    vis, tac = s.get("vision", True), s.get("tactile", True) and s["k"] > 0
    whole = B // 2 if B > 1 else None
    image = _frames(gen, B, s["Ci"], s["img"], s["Pi"], whole if not tac else None) if vis else None
    tactiles = [_frames(gen, B, s["Ct"], s["tac"], s["Pt"], whole if i == s["k"] - 1 else None) for i in range(s["k"])] if tac else []
    return image, tactiles


def _rn(gen, *shape, scale=1.0, shift=0.0):
    return (shift + scale * torch.randn(*shape, generator=gen)).float()


def _cuda(t, dev, grad=False):
    if t is None:
        return None
    t = t.detach().clone().to(dev)
    return t.requires_grad_(True) if grad else t


def _ref_leaf(t, grad=True):
    return None if t is None else t.to(F64).requires_grad_(grad)


def _rnd_of(emu):
    return R.bf16_rnd if emu else R.ident


def _hgrads(out, cot, tensors):
    live = [t for t in tensors if t is not None and t.requires_grad]
    g = iter(torch.autograd.grad(out, live, cot, allow_unused=True))
    return [next(g) if (t is not None and t.requires_grad) else None for t in tensors]


def _absent(H, X, what):
    """a tensor that takes no gradient in the reference takes none (or zeros) from the kernels"""
    assert X is None and (H is None or float(H.abs().max()) == 0.0), what


# -------------------------------------------------------------------------------------------------------------------
# mask sampling: bit-exact against the stable argsort
def _mask_geom(n, k, vision):
    return _geom_of(dict(img=(8, 8 * n), tac=(4, 4 * n), Pi=8, Pt=4, Ci=3, Ct=3, k=k, vision=vision))


@pytest.mark.parametrize("k,vision", [(0, True), (1, True), (2, True), (8, True), (1, False), (2, False), (8, False)])
@pytest.mark.parametrize("n", [1, 16, 64, 196, 257, 784])      # 64 / 128 / 256 threads per row; 257 and 784: several keys per thread
def test_mask_sample(dev, n, k, vision):
    geom = _mask_geom(n, k, vision)
    gen = _gen(f"mask{n}.{k}.{vision}")
    B = 5
    noises = []
    for i in range((1 if vision else 0) + k):
        z = torch.floor(torch.rand(B, n, generator=gen) * 8) / 8            # 8 levels: ties in every row longer than 8
        z[1] = 0.25                                                        # an all-equal row
        z[2, ::2] = -0.0                                                   # -0.0 and +0.0 compare equal: index order decides
        z[2, 1::2] = 0.0
        z[3] = torch.rand(n, generator=gen)                                # a tie-free row
        noises.append(z)
    for ratio, counts in ((0.75, None), (0.5, (0, 0)), (0.5, (n if vision else 0, n if k else 0)), (0.95, None)):
        mr, ur, cr = R.mask_sample(geom, ratio, [z.numpy() for z in noises], counts)
        mh, uh, ch = Fn.mask_sample(geom, ratio, [z.to(dev) for z in noises], counts)
        assert ch == cr, (ch, cr)
        check_exact("mask_sample", "int", f"masked n={n} k={k} r={ratio} counts={counts}", mh, mr)
        check_exact("mask_sample", "int", f"unmasked n={n} k={k} r={ratio} counts={counts}", uh, ur)


# -------------------------------------------------------------------------------------------------------------------
# patch embed
# patch dims: 192 / 48 (<= 256: NV = 4), 2352 / 588 (> 1024: NV = 40, and <= 1024: NV = 16), 147 / 75 (pd % 4 != 0: the element-wise walk)
EMBED = {
    "p8x4_D64_k2": dict(img=32, tac=16, Pi=8, Pt=4, Ci=3, Ct=3, k=2, D=64, B=3),
    "p14_D192_k1": dict(img=28, tac=28, Pi=14, Pt=14, Ci=12, Ct=3, k=1, D=192, B=2),
    "p7p5_D384_k4": dict(img=21, tac=10, Pi=7, Pt=5, Ci=3, Ct=3, k=4, D=384, B=2),       # k = 4: nslot > 2, the three-launch reduce
    "vision_only": dict(img=32, tac=16, Pi=8, Pt=4, Ci=3, Ct=3, k=2, D=64, B=3, tactile=False),
    "tactile_only": dict(img=32, tac=16, Pi=8, Pt=4, Ci=3, Ct=3, k=2, D=64, B=3, vision=False),
    "learned_pos": dict(img=32, tac=16, Pi=8, Pt=4, Ci=3, Ct=3, k=2, D=64, B=3, learned=True),
    # 4483 samples of 2 + 2 patches.  All patches: 8966 rows per group; visible list (1 + 1 per sample): 4480 + 3 rows per group.  Either
    # way the partial-sum kernels (patch_ln_bwd, embed_finalize_bwd, colsum) loop over their 1024-block grid and end on a ragged block
    "rows4483": dict(img=(8, 16), tac=(4, 8), Pi=8, Pt=4, Ci=3, Ct=3, k=1, D=64, B=4483, counts=(1, 1)),
    # m3l_colsum (the projection's bias gradient) has no threshold at 4096 rows: a block owns 64 rows (16 for matrices wider than 512) until
    # that would take more than 1024 blocks, i.e. from 65 537 rows on.  65 540 one-patch samples reach it (65 rows per block) — and 17 rows
    # per wave in the other partial-sum kernels
    "rows65540": dict(img=8, tac=4, Pi=8, Pt=4, Ci=3, Ct=3, k=1, D=64, B=65540, vision=False, counts=(0, 0)),
    "one_row": dict(img=8, tac=16, Pi=8, Pt=4, Ci=3, Ct=3, k=1, D=64, B=1),             # the image group is ONE row
}


@functools.lru_cache(maxsize=None)
def _embed_data(name):
    s = EMBED[name]
    gen = _gen("embed." + name)
    geom = _geom_of(s)
    n_img, n_tac, k = R.geo(geom)
    D, B = s["D"], s["B"]
    pd = (s["Ci"] * s["Pi"] ** 2, s["Ct"] * s["Pt"] ** 2)
    tens = []
    for i in range(2):
        tens += [_rn(gen, pd[i], scale=0.5, shift=1.0), _rn(gen, pd[i], scale=0.4), _rn(gen, D, pd[i], scale=2 / math.sqrt(pd[i])),
                 _rn(gen, D, scale=0.4), _rn(gen, D, scale=0.5, shift=1.0), _rn(gen, D, scale=0.4)]
    tens += [_rn(gen, 1 + s["k"], D, scale=0.4), _rn(gen, max(n_img, 1), D, scale=0.5), _rn(gen, max(k * n_tac, 1), D, scale=0.5)]
    image, tactiles = _inputs(gen, s, B)
    noises = [torch.rand(B, n, generator=gen).numpy() for n in ([n_img] if n_img else []) + [n_tac] * k]
    _, unmasked, c = R.mask_sample(geom, 0.75, noises, s.get("counts"))
    return dict(s=s, geom=geom, tens=tens, image=image, tactiles=tactiles, unmasked=unmasked, c=c, N=n_img + k * n_tac, n_img=n_img)


def _embed_call(d, use_idx):
    idx = d["unmasked"] if use_idx else None
    cnt_img = d["c"]["n_img"] - d["c"]["nm_img"] if use_idx else d["n_img"]
    L_tok = d["unmasked"].shape[1] if use_idx else d["N"]
    return idx, cnt_img, L_tok


def _embed_grad_mask(d):
    """which of the 15 tensors take a gradient: everything, the position tables only when they are learned"""
    learned = bool(d["s"].get("learned"))
    return [True] * 13 + [learned, learned]


@functools.lru_cache(maxsize=None)
def _embed_cot(name, use_idx):
    d = _embed_data(name)
    _, _, L_tok = _embed_call(d, use_idx)
    return _rn(_gen(f"embed.cot.{name}.{use_idx}"), d["s"]["B"], L_tok, d["s"]["D"])


@functools.lru_cache(maxsize=None)
def _embed_ref(name, use_idx, emu, abs_cot=False):
    d = _embed_data(name)
    idx, cnt_img, L_tok = _embed_call(d, use_idx)
    tens = [_ref_leaf(t, g) for t, g in zip(d["tens"], _embed_grad_mask(d))]
    tok = R.embed(d["geom"], d["s"]["D"], idx, cnt_img, L_tok, d["image"], d["tactiles"], *tens, rnd=_rnd_of(emu))
    cot = _embed_cot(name, use_idx)
    return tok.detach(), R.grads_of(tok, cot.abs() if abs_cot else cot, tens)


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("use_idx", [False, True], ids=["all", "visible"])
@pytest.mark.parametrize("name", list(EMBED))
def test_embed(dev, name, use_idx, dt):
    d = _embed_data(name)
    s, D, B = d["s"], d["s"]["D"], d["s"]["B"]
    idx, cnt_img, L_tok = _embed_call(d, use_idx)
    tens = [_cuda(t, dev, g) for t, g in zip(d["tens"], _embed_grad_mask(d))]
    tokH = Fn.EmbedFn.apply(None, d["geom"], D, Fn.dtype_code(dt), _cuda(idx, dev), cnt_img, L_tok, _cuda(d["image"], dev),
                            [t.to(dev) for t in d["tactiles"]], *tens)
    gH = _hgrads(tokH, _embed_cot(name, use_idx).to(dev), tens)
    tokX, gX = _embed_ref(name, use_idx, False)
    tokR, gR = _embed_ref(name, use_idx, True) if dt == "bf16" else (None, [None] * 15)
    _, gA = _embed_ref(name, use_idx, False, True)       # the same sums over |cotangent|: sum|terms| of the bias / modality / position sums
    stage, tag = "embed", f"{name}/{'visible' if use_idx else 'all'}"
    check_val(stage, dt, f"{tag} tokens", tokH, tokX, tokR)
    rows = (B * cnt_img, B * (L_tok - cnt_img))
    names = ["ln1_w", "ln1_b", "W", "b", "ln2_w", "ln2_b"]
    for i in range(12):
        what = f"{tag} {'image' if i < 6 else 'tactile'}.{names[i % 6]}"
        if gX[i] is None:
            _absent(gH[i], gX[i], what)
        elif i % 6 == 5:
            # second LayerNorm's bias gradient = column sums of the f32 cotangent over the group's rows (embed_finalize_bwd_kernel)
            check_sum(stage, dt, what, gH[i], gX[i], gA[i], _chain(rows[i // 6]))
        else:
            check_val(stage, dt, what, gH[i], gX[i], gR[i])
    # modality rows: the same kernel, one slot per sensor; a row sums the cotangent rows of its sensor only, the chain is that of the group
    check_sum(stage, dt, f"{tag} mod", gH[12], gX[12], gA[12], max(_chain(r) for r in rows if r))
    for i in (13, 14):
        if gX[i] is None:
            _absent(gH[i], gX[i], f"{tag} pos{i}")
        else:      # learned positions: Fn._pos_grads scatters (a copy) and adds the B samples (torch.sum over dim 0: at most B - 1 additions)
            check_sum(stage, dt, f"{tag} pos{i}", gH[i], gX[i], gA[i], B)


# -------------------------------------------------------------------------------------------------------------------
# token assembly behind the EarlyCNN stems (f32 only: nothing is stored in a compute type)
ASSEMBLE = {      # B = 70 at N = 80: 5600 rows > 4096, the backward loops over its grid
    "k1_B1_D64": dict(img=32, tac=16, Pi=8, Pt=4, Ci=3, Ct=3, k=1, D=64, B=1),
    "k2_B70_D256": dict(img=32, tac=16, Pi=8, Pt=4, Ci=3, Ct=3, k=2, D=256, B=70),
    "k4_B70_D64": dict(img=32, tac=16, Pi=8, Pt=4, Ci=3, Ct=3, k=4, D=64, B=70),
    "k4_B1_D256_learned": dict(img=32, tac=16, Pi=8, Pt=4, Ci=3, Ct=3, k=4, D=256, B=1, learned=True),
}


@pytest.mark.parametrize("name", list(ASSEMBLE))
def test_tokens_assemble(dev, name):
    s = ASSEMBLE[name]
    gen = _gen("assemble." + name)
    geom = _geom_of(s)
    n_img, n_tac, k = R.geo(geom)
    D, B, N = s["D"], s["B"], n_img + k * n_tac
    learned = bool(s.get("learned"))
    cpu = [_rn(gen, B, n_img, D), _rn(gen, k * B, n_tac, D), _rn(gen, 1 + k, D, scale=0.4), _rn(gen, n_img, D, scale=0.5), _rn(gen, k * n_tac, D, scale=0.5)]
    gmask = [True, True, True, learned, learned]
    cot = _rn(gen, B, N, D)
    th = [_cuda(t, dev, g) for t, g in zip(cpu, gmask)]
    tokH = Fn.TokensAssembleFn.apply(None, geom, D, *th)
    gH = _hgrads(tokH, cot.to(dev), th)
    tx = [_ref_leaf(t, g) for t, g in zip(cpu, gmask)]
    tokX = R.tokens_assemble(geom, D, *tx)
    gX = R.grads_of(tokX, cot, tx)
    gA = R.grads_of(tokX, cot.abs(), tx)
    tokA = R.tokens_assemble(geom, D, *[t.detach().abs() for t in tx])
    stage, dt = "tokens_assemble", "fp32"
    check_sum(stage, dt, f"{name} tokens", tokH, tokX, tokA, 2)                  # src + mod + pos: two additions
    check_exact(stage, dt, f"{name} d_img", gH[0], gX[0].float())               # copies of the cotangent rows
    check_exact(stage, dt, f"{name} d_tac", gH[1], gX[1].float())
    check_sum(stage, dt, f"{name} dmod", gH[2], gX[2], gA[2], _chain(B * N))     # tokens_assemble_bwd_kernel: one slot per modality
    for i in (3, 4):
        if learned:
            check_sum(stage, dt, f"{name} pos{i}", gH[i], gX[i], gA[i], B)
        else:
            assert gH[i] is None


# -------------------------------------------------------------------------------------------------------------------
# encoder -> decoder glue
UNSHUFFLE = {
    # N = 16 + 2 * 9 = 34 (no multiple of 16): a wave's run of 16 rows crosses modality and sample boundaries
    "proj_128_64_k2": dict(img=32, tac=12, Pi=8, Pt=4, Ci=3, Ct=3, k=2, D=128, dd=64, B=3, proj=True),
    "proj_learned": dict(img=32, tac=12, Pi=8, Pt=4, Ci=3, Ct=3, k=2, D=128, dd=64, B=3, proj=True, learned=True),
    "dd64_k4": dict(img=32, tac=12, Pi=8, Pt=4, Ci=3, Ct=3, k=4, D=64, dd=64, B=5),              # MAXC 1; nmod = 5 > 3: the two-launch reduce
    "dd64_k4_vis1000": dict(img=32, tac=12, Pi=8, Pt=4, Ci=3, Ct=3, k=4, D=64, dd=64, B=5, vis_scale=1000.0),
    "dd384_k1": dict(img=32, tac=12, Pi=8, Pt=4, Ci=3, Ct=3, k=1, D=384, dd=384, B=2),           # MAXC 2
    "dd768_k0": dict(img=32, tac=12, Pi=8, Pt=4, Ci=3, Ct=3, k=2, D=768, dd=768, B=2, tactile=False),      # MAXC 4, vision only
    # B N = 1600 * 42 = 67 200 > 65 536: rows per wave doubles to 32 (k_unshuffle_bwd); N = 6 + 4 * 9
    "rows67200": dict(img=(16, 24), tac=12, Pi=8, Pt=4, Ci=3, Ct=3, k=4, D=64, dd=64, B=1600),
}


@functools.lru_cache(maxsize=None)
def _unshuffle_data(name, dt):
    s = UNSHUFFLE[name]
    gen = _gen("unshuffle." + name)
    geom = _geom_of(s)
    n_img, n_tac, k = R.geo(geom)
    D, dd, B, N = s["D"], s["dd"], s["B"], n_img + k * n_tac
    noises = [torch.rand(B, n, generator=gen).numpy() for n in [n_img] + [n_tac] * k]
    masked, unmasked, c = R.mask_sample(geom, 0.75, noises)
    nvis = unmasked.shape[1]
    proj = bool(s.get("proj"))
    tens = [_rn(gen, dd, D, scale=2 / math.sqrt(D)) if proj else None, _rn(gen, dd, scale=0.4) if proj else None, _rn(gen, dd, scale=0.4),
            _rn(gen, 1 + s["k"], dd, scale=0.4), _rn(gen, n_img, dd, scale=0.5), _rn(gen, max(k * n_tac, 1), dd, scale=0.5)]
    enc = _rn(gen, B, nvis, D)
    if dt == "bf16":           # the encoder output arrives in the compute type: rounded before either side sees it
        enc = enc.to(torch.bfloat16).float()
    cot = _rn(gen, B, N, dd)
    if s.get("vis_scale"):     # visible rows dominate: dmask_token = (sum of all rows) - (sum of visible rows) cancels three digits
        cot[torch.arange(B)[:, None], unmasked] *= s["vis_scale"]
    learned = bool(s.get("learned"))
    return dict(s=s, geom=geom, tens=tens, enc=enc, cot=cot, masked=masked, unmasked=unmasked, N=N, proj=proj,
                gmask=[proj, proj, True, True, learned, learned])


@functools.lru_cache(maxsize=None)
def _unshuffle_ref(name, dt, emu, abs_mode=False):
    d = _unshuffle_data(name, dt)
    s = d["s"]
    tens = [_ref_leaf(t, g) for t, g in zip(d["tens"], d["gmask"])]
    enc = _ref_leaf(d["enc"])
    if abs_mode:       # sum|terms| of dec_in = src + mod + pos (no projection), and of the gradients that are plain sums of cotangent rows
        tens = [None if t is None else t.detach().abs().requires_grad_(t.requires_grad) for t in tens]
        enc = enc.detach().abs().requires_grad_(True)
    out = R.unshuffle(d["geom"], s["D"], s["dd"], d["unmasked"], d["masked"], enc, enc, *tens, rnd=_rnd_of(emu))
    g = R.grads_of(out, d["cot"].abs() if abs_mode else d["cot"], [enc] + tens)
    return out.detach(), g


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("name", list(UNSHUFFLE))
def test_unshuffle(dev, name, dt):
    d = _unshuffle_data(name, dt)
    s, proj = d["s"], d["proj"]
    D, dd, B, N = s["D"], s["dd"], s["B"], d["N"]
    nvis = d["unmasked"].shape[1]
    code = Fn.dtype_code(dt)
    tens = [_cuda(t, dev, g) for t, g in zip(d["tens"], d["gmask"])]
    enc32 = _cuda(d["enc"], dev, True)
    enc_t = _cuda(d["enc"].to(Fn.tdtype(code)).clone(), dev, True)
    um, mm = d["unmasked"].to(dev), d["masked"].to(dev)
    outH = Fn.UnshuffleFn.apply(None, d["geom"], D, dd, code, um, mm, enc_t, enc32, *tens)
    gH = _hgrads(outH, d["cot"].to(dev), [enc_t, enc32] + tens)
    d_encH = gH[0] if proj else gH[1]
    assert (gH[1] if proj else gH[0]) is None
    gH = [d_encH] + gH[2:]
    outX, gX = _unshuffle_ref(name, dt, False)
    outR, gR = _unshuffle_ref(name, dt, True) if (dt == "bf16" and proj) else (None, [None] * 7)
    stage = "unshuffle"
    rows = B * N
    # k_unshuffle_bwd: rows per wave 16, doubled while more than 1024 blocks of 4 waves would be needed; vpw visible rows per wave
    rpw = 16
    while ((rows + rpw - 1) // rpw + 3) // 4 > 1024:
        rpw *= 2
    G = ((rows + rpw - 1) // rpw + 3) // 4
    vpw = (B * nvis + 4 * G - 1) // (4 * G)
    assert (rpw == 32) == (name == "rows67200"), rpw
    # unshuffle_bwd_kernel: a wave adds its run of rows (at most rpw additions), flushes once per modality segment of the run (at most rpw
    # more), adds its visible rows (vpw) and flushes; the four waves' slabs (3); then the reduction over the G partial rows
    c_bwd = 2 * rpw + vpw + 1 + 3 + _reduce_chain(G)
    if proj:
        check_val(stage, dt, f"{name} dec_in", outH, outX, outR)
        check_val(stage, dt, f"{name} d_enc", gH[0], gX[0], gR[0])
        check_val(stage, dt, f"{name} e2d_w", gH[1], gX[1], gR[1])
        # bias gradient: m3l_colsum over the UNROUNDED f32 dsrc: a block of rpb rows in four chains (rpb / 4 + 2 <= rpb), then the reduction
        Mv = B * nvis
        Gc = min((Mv + 63) // 64, 1024)
        rpb = (Mv + Gc - 1) // Gc
        _, gA = _unshuffle_ref(name, dt, False, True)
        check_sum(stage, dt, f"{name} e2d_b", gH[2], gX[2], gA[2], rpb + _reduce_chain((Mv + rpb - 1) // rpb))
    else:
        outA, gA = _unshuffle_ref(name, dt, False, True)
        check_sum(stage, dt, f"{name} dec_in", outH, outX, outA, 2)                 # src + mod + pos
        check_exact(stage, dt, f"{name} d_enc", gH[0], gX[0].float())                # the f32 gather itself
        assert gH[1] is None and gH[2] is None
    cotA = d["cot"].to(F64).abs()
    vis_abs = cotA[torch.arange(B)[:, None], d["unmasked"]].sum((0, 1))
    # dmask_token is formed as (all rows) - (visible rows): both sets are its terms
    check_sum(stage, dt, f"{name} mask_token", gH[3], gX[3], cotA.sum((0, 1)) + vis_abs, c_bwd)
    check_sum(stage, dt, f"{name} dec_mod", gH[4], gX[4], gA[4], c_bwd)
    for i in (5, 6):
        if d["gmask"][i - 1]:
            check_sum(stage, dt, f"{name} pos{i}", gH[i], gX[i], gA[i], B)
        else:
            assert gH[i] is None


# -------------------------------------------------------------------------------------------------------------------
# heads + masked MSE
HEADS = {
    "p8x4_dd64": dict(img=32, tac=16, Pi=8, Pt=4, Ci=3, Ct=3, k=2, dd=64, B=3),
    "p14_dd128": dict(img=28, tac=28, Pi=14, Pt=14, Ci=12, Ct=3, k=1, dd=128, B=2),
    "p7p5_dd64": dict(img=21, tac=10, Pi=7, Pt=5, Ci=3, Ct=3, k=4, dd=64, B=2),
    "vision_only": dict(img=32, tac=16, Pi=8, Pt=4, Ci=3, Ct=3, k=2, dd=64, B=3, tactile=False),
    "tactile_only": dict(img=32, tac=16, Pi=8, Pt=4, Ci=3, Ct=3, k=2, dd=64, B=3, vision=False),
    "early_conv": dict(img=32, tac=16, Pi=8, Pt=4, Ci=3, Ct=3, k=2, dd=64, B=3, all_rows=True),      # identity index list over all N rows
    # 400 samples x 12 masked image patches = 4800 rows > 4096 in the image group: mse_kernel and the bias column sums loop over their grid
    "rows4800": dict(img=32, tac=8, Pi=8, Pt=4, Ci=3, Ct=3, k=1, dd=64, B=400),
}
HEAD_RUNS = [(n, 0.37) for n in HEADS] + [("p8x4_dd64", 1.0), ("p8x4_dd64", 1024.0)]


@functools.lru_cache(maxsize=None)
def _heads_data(name, dt):
    s = HEADS[name]
    gen = _gen("heads." + name)
    geom = _geom_of(s)
    n_img, n_tac, k = R.geo(geom)
    dd, B, N = s["dd"], s["B"], n_img + k * n_tac
    pd = (s["Ci"] * s["Pi"] ** 2, s["Ct"] * s["Pt"] ** 2)
    tens = [_rn(gen, pd[0], dd, scale=2 / math.sqrt(dd)), _rn(gen, pd[0], scale=0.4), _rn(gen, pd[1], dd, scale=2 / math.sqrt(dd)), _rn(gen, pd[1], scale=0.4)]
    image, tactiles = _inputs(gen, s, B)
    noises = [torch.rand(B, n, generator=gen).numpy() for n in ([n_img] if n_img else []) + [n_tac] * k]
    masked, _, c = R.mask_sample(geom, 0.75, noises)
    nm_img = c["nm_img"]
    if s.get("all_rows"):
        masked, nm_img = torch.arange(N).expand(B, N).contiguous(), n_img
    dec = _rn(gen, B, N, dd)
    if dt == "bf16":
        dec = dec.to(torch.bfloat16).float()
    return dict(s=s, geom=geom, tens=tens, image=image, tactiles=tactiles, masked=masked, nm_img=nm_img, dec=dec, N=N, n_img=n_img, k=k)


@functools.lru_cache(maxsize=None)
def _heads_ref(name, dt, dloss, emu):
    d = _heads_data(name, dt)
    with torch.no_grad():
        return R.heads_loss(d["geom"], d["s"]["dd"], d["masked"], d["nm_img"], d["image"], d["tactiles"], d["dec"], *d["tens"], dloss=dloss,
                            rnd=_rnd_of(emu))


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("name,dloss", HEAD_RUNS)
def test_heads_loss(dev, name, dloss, dt):
    d = _heads_data(name, dt)
    s, dd, B, N = d["s"], d["s"]["dd"], d["s"]["B"], d["N"]
    code = Fn.dtype_code(dt)
    has = (d["n_img"] > 0, d["k"] > 0)
    tens = [_cuda(t, dev, True) for t in d["tens"]]
    dec_t = _cuda(d["dec"].to(Fn.tdtype(code)), dev, True)
    masked = d["masked"].to(dev)
    dump = {}
    lossH = Fn.HeadsLossFn.apply(None, d["geom"], dd, code, masked, d["nm_img"], _cuda(d["image"], dev), [t.to(dev) for t in d["tactiles"]], dump,
                                 dec_t, *tens)
    gH = _hgrads(lossH, torch.tensor(dloss, device=dev), [dec_t] + tens)
    X = _heads_ref(name, dt, dloss, False)
    Rr = _heads_ref(name, dt, dloss, True) if dt == "bf16" else None
    rr = (lambda key: Rr[key]) if Rr is not None else (lambda key: None)
    stage, tag = "heads_loss", f"{name}/dloss={dloss:g}"
    check_val(stage, dt, f"{tag} loss", lossH, X["loss"], rr("loss"))
    check_val(stage, dt, f"{tag} loss_parts", dump["loss_parts"], X["loss_parts"], rr("loss_parts"))
    pats = R.patches_of(d["geom"], d["image"], d["tactiles"])
    br = torch.arange(B)[:, None]
    for gi, key in enumerate(("pixel", "tactile")):
        if not has[gi]:
            assert dump["pred_" + key].numel() == 0
            _absent(gH[1 + 2 * gi], None, f"{tag} {key} W")
            _absent(gH[2 + 2 * gi], None, f"{tag} {key} b")
            continue
        check_val(stage, dt, f"{tag} pred_{key}", dump["pred_" + key], X["pred_" + key], None if Rr is None else Rr["pred_" + key])
        # the targets are the raw f32 patches, bit for bit
        rows = d["masked"][:, :d["nm_img"]] if gi == 0 else d["masked"][:, d["nm_img"]:] - d["n_img"]
        check_exact(stage, dt, f"{tag} target_{key}", dump["target_" + key], pats[gi][br, rows].float())
        check_val(stage, dt, f"{tag} {key} W", gH[1 + 2 * gi], X["grads"][2 * gi], None if Rr is None else Rr["grads"][2 * gi])
        check_val(stage, dt, f"{tag} {key} b", gH[2 + 2 * gi], X["grads"][2 * gi + 1], None if Rr is None else Rr["grads"][2 * gi + 1])
    check_val(stage, dt, f"{tag} d_dec", gH[0], X["d_dec"], rr("d_dec"))
    vis = torch.ones(B, N, dtype=torch.bool)
    vis[br, d["masked"]] = False
    if vis.any():
        assert float(gH[0].detach().cpu()[vis].float().abs().max()) == 0.0, f"{tag}: d_dec is not exactly zero on the visible rows"
    else:
        assert s.get("all_rows")


# -------------------------------------------------------------------------------------------------------------------
# token gather / scatter: bit-equal to torch indexing
@pytest.mark.parametrize("B,N,D,K", [(3, 37, 100, 1), (3, 37, 100, 37), (2, 16, 64, 5), (1, 1, 8, 1), (5, 130, 384, 130)])
def test_gather_scatter(dev, B, N, D, K):
    gen = _gen(f"gather{B}.{N}.{D}.{K}")
    x = _rn(gen, B, N, D)
    idx = torch.stack([torch.randperm(N, generator=gen)[:K] for _ in range(B)])       # unique per sample: the scatter's contract
    cot = _rn(gen, B, K, D)
    xh = _cuda(x, dev, True)
    yh = Fn.GatherTokensFn.apply(xh, idx.to(dev))
    (dxh,) = torch.autograd.grad(yh, [xh], cot.to(dev))
    check_exact("gather_scatter", "fp32", f"gather {B}x{N}x{D} K={K}", yh, R.gather_tokens(x, idx))
    check_exact("gather_scatter", "fp32", f"scatter {B}x{N}x{D} K={K}", dxh, R.scatter_tokens(cot, idx, N))
