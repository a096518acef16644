"""float64 restatement of the MAE step's stage kernels, one function per stage.  *** TEST INFRASTRUCTURE ONLY ***

The stages are what sits around the two transformer stacks of VTMAE.forward (reference models/pretrain_models.py):

  mask_sample      :223-248   per-modality argsort of injected noise (stable ascending), masked / visible lists in concat order
  embed            :157-216, 255-256   patchify -> LayerNorm -> Linear -> LayerNorm + modality + position, all patches or a visible list
  tokens_assemble  :202-216   the same "+ modality + position" behind the EarlyCNN stems (stem tokens arrive sensor-major)
  unshuffle        :270-307   enc_to_dec, un-shuffle into position order, mask token, decoder modality + position
  heads_loss       :260-262, 327-340   masked-row gather, to_pixels / to_tactiles, mse(image) + 10 mse(tactile)
  gather_tokens / scatter_tokens   tokens[batch_range, idx] and its adjoint

Plain CPU torch in float64; the backward is autograd (heads_loss writes its few lines out, because the upstream gradient `dloss` enters
AFTER two of the bf16 roundings).  The argument order is that of the matching m3l_amd.functional.*Fn without `sink` and the dtype code.
tests/test_stage_refs_cpu.py anchors these functions to oracle/vtmae_oracle.py (1e-12) and to the reference's own recorded run.

`rnd` (default: identity) is applied wherever the bf16 plan of m3l_amd/csrc/mae_plan.hip STORES a tensor in the compute type; with
`rnd = bf16_rnd` a function is the emulated-bf16 reference (float64 arithmetic between the storage points).  The storage points, each
read off the code (struct names are those of mae_plan.hip):

  embed (embed_run)
    EmbGroupWs::w / wT   the projection weight, both copies (m3l_prep_weight_list): forward GEMM and dxn GEMM
    EmbGroupWs::xn       output of the first LayerNorm (patch_ln_kernel stores T); operand of the forward GEMM and of dW
    EmbGroupWs::E        stays f32 (GemmEpi::out_f32) — NOT rounded
    EmbGroupWs::dE       backward of the second LayerNorm (embed_finalize_bwd_kernel stores T); operand of dW, of the bias column sums
                         (m3l_colsum reads dE in the compute type) and of the dxn GEMM
    EmbGroupWs::dxn      GemmEpi::out_t; patch_ln_bwd_kernel forms dgamma / dbeta of the first LayerNorm from it and from statistics
                         recomputed in f32 from the raw patches
    the second LayerNorm's dgamma / dbeta and the modality / position gradients are sums of the f32 dtokens: downstream of no rounding
  unshuffle with enc_to_dec (m3l_unshuffle_fwd / _bwd)
    UnWs::w / wT         the projection weight
    UnWs::proj           f32 — not rounded
    UnWs::dsrc           f32 gather of d_dec_in: the bias gradient is m3l_colsum(0, dsrc): unrounded
    UnWs::dsrc_t         m3l_cast_f32 of dsrc: operand of dW and of the d_enc GEMM
    d_enc                GemmEpi::out_t
    without enc_to_dec nothing is rounded: d_enc is the f32 gather itself
  heads (m3l_heads_loss_fwd2 / _bwd)
    HeadGroupWs::w / wT  the head weight
    HeadGroupWs::pred    f32 — not rounded; the loss is formed from it
    HeadGroupWs::dpred   = 2 w (pred - tgt), w = weight / (rows pd) (mse_kernel stores T)
    HeadGroupWs::dpred_s = dpred * dloss (m3l_scale_by_dev): operand of dW and of the bias column sums
    HeadGroupWs::ddg     = dpred W (GemmEpi::out_t), from the UNSCALED dpred
    d_dec                = ddg * dloss, rounded again by scatter_rows2_kernel; exactly zero on rows no index names
  enc_t / dec_t arrive in the compute type: the caller rounds them before either side sees them.
"""
from types import SimpleNamespace

import numpy as np
import torch
import torch.nn.functional as F

F64 = torch.float64
LN_EPS = 1e-5


def ident(t):
    return t


def bf16_rnd(t):
    """round-to-nearest-even to bfloat16, back in float64 (|t| < 2^127: float64 -> float32 -> bf16 double rounding can differ from a
    direct rounding only on exact float32 ties, which the kernels — f32 registers — round the same way)"""
    return t.to(torch.float32).to(torch.bfloat16).to(F64)


def make_geom(image_hw, image_patch, image_channels, tactile_hw, tactile_patch, tactile_channels, num_tactiles, use_vision=True, use_tactile=True):
    """the fields of m3l_geom (an m3l_amd._lib.Geom works wherever this does)"""
    return SimpleNamespace(image_h=image_hw, image_w=image_hw, image_patch=image_patch, image_channels=image_channels,
                           tactile_h=tactile_hw, tactile_w=tactile_hw, tactile_patch=tactile_patch, tactile_channels=tactile_channels,
                           num_tactiles=int(num_tactiles), use_vision=int(bool(use_vision)), use_tactile=int(bool(use_tactile)))


def geo(g):
    """active counts of a call: (n_img, n_tac, k), 0 for a modality that is absent from it"""
    n_img = (g.image_h // g.image_patch) * (g.image_w // g.image_patch) if g.use_vision else 0
    k = g.num_tactiles if (g.use_tactile and g.num_tactiles > 0) else 0
    n_tac = (g.tactile_h // g.tactile_patch) * (g.tactile_w // g.tactile_patch) if k else 0
    return n_img, n_tac, k


def mask_counts(g, ratio):
    """:223-227, Python double arithmetic with int() truncation"""
    n_img, n_tac, k = geo(g)
    n = n_img + k * n_tac
    num_masked = int(ratio * n)
    nm_img = int(num_masked * (n_img / n))
    nm_tac = (num_masked - nm_img) // k if k else 0
    total = nm_img + k * nm_tac
    return dict(num_masked=total, num_unmasked=n - total, nm_img=nm_img, nm_tac=nm_tac, n_img=n_img, n_tac=n_tac)


def mask_sample(geom, ratio, noises, counts=None):
    """noises: (B, n_i) arrays in RNG order image, tactile1..k -> int64 (masked, unmasked, counts dict).  Ascending, ties by ascending index."""
    c = mask_counts(geom, ratio)
    n_img, n_tac, k = geo(geom)
    if counts is not None:
        c = dict(c, nm_img=counts[0], nm_tac=counts[1], num_masked=counts[0] + k * counts[1])
        c["num_unmasked"] = n_img + k * n_tac - c["num_masked"]
    noises = [np.asarray(n) for n in noises]
    masked, unmasked, i, off = [], [], 0, 0
    for n, nm in ([(n_img, c["nm_img"])] if n_img else []) + [(n_tac, c["nm_tac"])] * k:
        assert noises[i].shape[1] == n
        perm = np.argsort(noises[i], axis=-1, kind="stable").astype(np.int64) + off
        masked.append(perm[:, :nm])
        unmasked.append(perm[:, nm:])
        i, off = i + 1, off + n
    return torch.from_numpy(np.concatenate(masked, 1)), torch.from_numpy(np.concatenate(unmasked, 1)), c


# -------------------------------------------------------------------------------------------------------------------
class _Stored(torch.autograd.Function):
    """a tensor the forward stores in the compute type; its gradient passes unchanged (the f32 master takes the gradient)"""

    @staticmethod
    def forward(ctx, t, rnd):
        return rnd(t)

    @staticmethod
    def backward(ctx, g):
        return g, None


class _GradStored(torch.autograd.Function):
    """identity whose incoming gradient is stored in the compute type before anything reads it"""

    @staticmethod
    def forward(ctx, t, rnd):
        ctx.rnd = rnd
        return t.view_as(t)

    @staticmethod
    def backward(ctx, g):
        return ctx.rnd(g), None


def _f64(t):
    return None if t is None else (t if t.dtype == F64 else t.to(F64))


def patchify(x, p):
    """'b c (h p1) (w p2) -> b (h w) (p1 p2 c)'"""
    B, C, H, W = x.shape
    return x.reshape(B, C, H // p, p, W // p, p).permute(0, 2, 4, 3, 5, 1).reshape(B, (H // p) * (W // p), p * p * C)


def _rows(t, idx):
    return t[torch.arange(t.shape[0])[:, None], idx]


def patches_of(geom, image, tactiles):
    """(image patches (B, n_img, pd_i) or None, tactile patches (B, k n_tac, pd_t) or None), float64, sensors concatenated in order"""
    n_img, n_tac, k = geo(geom)
    pi = patchify(_f64(image), geom.image_patch) if n_img else None
    pt = torch.cat([patchify(_f64(t), geom.tactile_patch) for t in tactiles[:k]], 1) if k else None
    return pi, pt


def embed(geom, D, idx, cnt_img, L_tok, image, tactiles, *tensors, rnd=ident):
    """tensors: image {ln1_w, ln1_b, W[D,pd], b, ln2_w, ln2_b}, tactile {same 6}, mod[(1+k),D], pos_img[n_img,D], pos_tac[k n_tac,D].
    idx None: all patches; else (B, L_tok) token numbers, the first cnt_img of each row image tokens.  -> tokens (B, L_tok, D)"""
    n_img, n_tac, k = geo(geom)
    t = [_f64(x) for x in tensors]
    mod, pos = t[12], (t[13], t[14])
    pats = patches_of(geom, image, tactiles)
    B = (image if n_img else tactiles[0]).shape[0]
    if idx is None:
        assert L_tok == n_img + k * n_tac and cnt_img == n_img
    out = []
    for gi, (lo, cnt, base) in enumerate(((0, cnt_img, 0), (cnt_img, L_tok - cnt_img, n_img))):
        if cnt == 0:
            continue
        ln1_w, ln1_b, W, b, ln2_w, ln2_b = t[6 * gi: 6 * gi + 6]
        local = (torch.arange(cnt).expand(B, cnt) if idx is None else idx[:, lo:lo + cnt] - base)
        p = _rows(pats[gi], local)
        xn = F.layer_norm(p, (p.shape[-1],), ln1_w, ln1_b, LN_EPS)
        xn = _GradStored.apply(_Stored.apply(xn, rnd), rnd)                 # xn stored; its gradient dxn stored
        E = xn @ _Stored.apply(W, rnd).t() + b                              # W stored (both copies hold the same values); E stays f32
        E = _GradStored.apply(E, rnd)                                       # dE stored: dW, db and dxn all read the stored dE
        tok = F.layer_norm(E, (D,), ln2_w, ln2_b, LN_EPS)
        m = mod[0].expand(B, cnt, D) if gi == 0 else mod[1 + local // n_tac]
        out.append(tok + m + pos[gi][local])
    return torch.cat(out, 1)


def tokens_assemble(geom, D, img_tok, tac_tok, mod, pos_img, pos_tac, rnd=ident):
    """img_tok (B, n_img, D) or None, tac_tok (k B, n_tac, D) sensor-major or None -> (B, N, D).  Nothing is stored in the compute type."""
    n_img, n_tac, k = geo(geom)
    mod = _f64(mod)
    out = []
    if n_img:
        out.append(_f64(img_tok) + mod[0] + _f64(pos_img))
    if k:
        tt = _f64(tac_tok)
        B = tt.shape[0] // k
        tt = tt.reshape(k, B, n_tac, D).permute(1, 0, 2, 3).reshape(B, k * n_tac, D)
        out.append(tt + mod[1:1 + k].repeat_interleave(n_tac, 0) + _f64(pos_tac))
    return torch.cat(out, 1)


def unshuffle(geom, D, dd, unmasked, masked, enc_t, enc32, *tensors, rnd=ident):
    """tensors: {e2d_w[dd,D] or None, e2d_b or None, mask_token[dd], dec_mod[(1+k),dd], pos_img[n_img,dd], pos_tac[k n_tac,dd]}.
    With enc_to_dec the compute-type copy enc_t is projected, without it the f32 copy enc32 passes through.  -> dec_in (B, N, dd)"""
    n_img, n_tac, k = geo(geom)
    e2d_w, e2d_b, mask_token, dmod, pos_img, pos_tac = [_f64(x) for x in tensors]
    B, nvis = unmasked.shape
    nmask = masked.shape[1]
    N = nvis + nmask
    assert N == n_img + k * n_tac
    if e2d_w is not None:
        src = _GradStored.apply(_f64(enc_t), rnd)                           # d_enc stored
        src = _GradStored.apply(src @ _Stored.apply(e2d_w, rnd).t(), rnd)   # W stored; dsrc_t stored: operand of dW and of d_enc
        src = src + e2d_b                                                   # the bias gradient sums the unrounded dsrc
    else:
        assert D == dd
        src = _f64(enc32)
    br = torch.arange(B)[:, None]
    full = torch.zeros(B, N, dd, dtype=F64)
    full = full.index_put((br, unmasked), src)
    full = full.index_put((br, masked), _f64(mask_token).expand(B, nmask, dd))
    add = []
    if n_img:
        add.append(dmod[0] + pos_img)
    if k:
        add.append(dmod[1:1 + k].repeat_interleave(n_tac, 0) + pos_tac)
    return full + torch.cat(add, 0)


def heads_loss(geom, dd, masked, nm_img, image, tactiles, dec_t, *tensors, dloss=1.0, rnd=ident):
    """tensors {pix_w[pd_i,dd], pix_b, tac_w[pd_t,dd], tac_b}; masked (B, nmask) token numbers, the first nm_img of a row image tokens (the
    early-conv form passes every token: arange(N), nm_img = n_img).  Returns a dict: loss, loss_parts [mse(image), 10 mse(tactile)],
    pred_pixel / target_pixel / pred_tactile / target_tactile, d_dec (B, N, dd), grads [4] (None for an absent head)."""
    n_img, n_tac, k = geo(geom)
    t = [_f64(x) for x in tensors]
    dec = _f64(dec_t).detach()
    dloss = float(dloss)
    B, N, _ = dec.shape
    pats = patches_of(geom, image, tactiles)
    out = dict(loss=torch.zeros((), dtype=F64), loss_parts=torch.zeros(2, dtype=F64), grads=[None] * 4, d_dec=torch.zeros(B, N, dd, dtype=F64))
    br = torch.arange(B)[:, None]
    for gi, (lo, cnt, base, weight, name) in enumerate(((0, nm_img, 0, 1.0, "pixel"), (nm_img, masked.shape[1] - nm_img, n_img, 10.0, "tactile"))):
        if cnt == 0:
            continue
        W, b = t[2 * gi].detach(), t[2 * gi + 1].detach()
        rows = masked[:, lo:lo + cnt]
        dg = dec[br, rows]                                                  # gathered copy of the compute-type rows
        tgt = pats[gi][br, rows - base]
        Wr = rnd(W)                                                         # W stored
        pred = dg @ Wr.t() + b                                              # f32, not stored in the compute type
        w = weight / (B * cnt * tgt.shape[-1])
        part = w * ((pred - tgt) ** 2).sum()
        dpred = rnd(2.0 * w * (pred - tgt))                                 # dpred stored
        dpred_s = rnd(dpred * dloss)                                        # dpred_s stored: weight and bias gradients
        ddg = rnd(dpred @ Wr)                                               # ddg stored, from the unscaled dpred
        out["d_dec"][br, rows] = rnd(ddg * dloss)                           # rounded again at the scatter
        out["grads"][2 * gi] = dpred_s.reshape(-1, dpred_s.shape[-1]).t() @ dg.reshape(-1, dd)
        out["grads"][2 * gi + 1] = dpred_s.sum((0, 1))
        out["loss_parts"][gi] = part
        out["loss"] = out["loss"] + part
        out["pred_" + name], out["target_" + name] = pred, tgt
    return out


def gather_tokens(x, idx):
    """x (B, N, D), idx (B, K) -> (B, K, D)"""
    return _rows(x, idx)


def scatter_tokens(dy, idx, N):
    """adjoint of gather_tokens for unique indices: zeros (B, N, D) with row idx[b, j] = dy[b, j]"""
    B, K, D = dy.shape
    return torch.zeros(B, N, D, dtype=dy.dtype).index_put((torch.arange(B)[:, None], idx), dy)


def grads_of(out, cot, tensors):
    """d <out, cot> / d tensor for every tensor (None where one is None, takes no gradient or is unused)"""
    live = [x for x in tensors if x is not None and x.requires_grad]
    g = iter(torch.autograd.grad(out, live, _f64(cot), allow_unused=True, retain_graph=True))
    return [next(g) if (x is not None and x.requires_grad) else None for x in tensors]
