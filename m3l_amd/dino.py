"""DINO self-distillation pieces on the HIP kernels of m3l_amd/csrc/dino.hip: the projection head, the fused cross-entropy with its
teacher centre, and the teacher's moving average.

Drop-ins for `tactile_ssl/model/layers/dino_head.py` (DINOHead), `tactile_ssl/loss/dino_loss.py` (DINOLoss) and
`tactile_ssl/utils/ema.py` (update_moving_average) of the reference: same constructor arguments, parameter / buffer names and shapes,
seeded initial values and arithmetic.

  head : Linear + GELU(erf) per hidden layer, Linear, row L2 normalisation (eps 1e-12), y = x_n W^T with W[k] = g[k] v[k] / ||v[k]||.
         The MLP is the NT GEMM with its bias / GELU epilogues forwards and the TN GEMM, the column sums and the NT GEMM with the gelu'
         epilogue backwards; L2 normalisation and weight normalisation are kernels of their own.
  loss : sum_p sum_q mean_b( -sum_k T[q,b,k] log_softmax(S[p,b,:] / ts)[k] ), T = softmax((teacher - center) / tt), every (p, q) pair, not
         divided by the number of pairs.  Because each row of T sums to one this is
         mean_b( Q sum_p lse(S[p,b,:] / ts) - 1/ts sum_k (sum_q T[q,b,k]) (sum_p S[p,b,k]) ), and
         dS[p,b,k] = g / (ts B) (Q softmax(S[p,b,:] / ts)[k] - sum_q T[q,b,k]): neither the P x Q products nor a log-softmax are stored.
  centre : the column sums of this step's teacher logits wait in `pending` and enter the centre at the start of the NEXT step
         (CenteredLoss.apply_center_update), so the first step runs with a zero centre.
  iBOT patch loss : the same cross-entropy, row by row, over the Q x (B n) patch rows of the global views (`tactile_ssl/loss/ibot_patch_loss.py`).
         Both terms take one path: RowFamily.args / loss_forward / loss_grad, the nodes RowLossFn and RowHeadLossFn (DinoLossFn, IbotLossFn,
         HeadLossFn and IbotHeadLossFn only name their family), and the centre state of CenteredLoss.  What differs is data, a RowFamily:
         DINO_ROWS (m3l_op_dino_*, a sample's teacher sums in LDS, B <= 255) or PATCH_ROWS
         (m3l_op_ibot_*, tiles over the rows, Q = P, Q R <= 65535), and in DINOLoss / iBOTPatchLoss the centre's shape and how its pending
         sums are formed (plain column sums over the rows; the split column sum scaled by samples / rows).
  Sinkhorn-Knopp : the teacher's other target (`centering="sinkhorn_knopp"`).  The reference scales exp(T / tt) to unit column and row sums
         n times; in the log domain that is u[k] = logsumexp_r(z[r,k] - w[r]), w[r] = logsumexp_k(z[r,k] - u[k]) from w = 0, and the
         targets are softmax((T - c) / tt) with c = tt u: one K-vector in the centre's place, no assignment matrix.  The u pass is the
         column kernel (m3l_op_sk_colstats / m3l_op_sk_colcombine), the w pass the row statistics the loss computes anyway.

There is no eager fallback: every number comes from a kernel, torch owns memory and the autograd tape.
"""
import ctypes as C
import math
from typing import Callable, NamedTuple

import torch
import torch.distributed as dist
from torch import nn
from torch.nn.init import trunc_normal_

from . import _lib as L
from .functional import DT_BF16, DT_F32, _f32c, _require_cuda, _stream, _ws, dtype_code, tdtype


def _cast(x, dt, transposed=False):
    """f32 (rows, cols) -> compute-type copy, or its transpose (cols, rows)."""
    rows, cols = x.shape
    if dt == DT_F32 and not transposed:
        return x
    out = torch.empty((cols, rows) if transposed else (rows, cols), dtype=tdtype(dt), device=x.device)
    L.check(L.lib().m3l_op_prep_weight(dt, L.ptr(x), rows, cols, None if transposed else L.ptr(out), L.ptr(out) if transposed else None,
                                       _stream()), "m3l_op_prep_weight")
    return out


def _gemm_nt(dt, a, w, M, N, K, bias=None, out_f32=None, out_t=None, out_pre=None, gelu_u=None, act=0):
    L.check(L.lib().m3l_op_gemm_nt(dt, L.ptr(a), K, L.ptr(w), K, M, N, K, L.ptr(bias), None, L.ptr(out_f32), L.ptr(out_t), L.ptr(out_pre),
                                   L.ptr(gelu_u), act, N, _stream()), "m3l_op_gemm_nt (DINO head)")


def _gemm_tn(dt, y, x, M, N, K):
    """dW (N, K) f32 = y^T x for y (M, N), x (M, K) in the compute type."""
    lib = L.lib()
    out = torch.empty(N, K, dtype=torch.float32, device=y.device)
    nb = lib.m3l_op_gemm_tn_ws_bytes(M, N, K)
    ws = _ws(nb, y.device)
    L.check(lib.m3l_op_gemm_tn(dt, L.ptr(y), N, L.ptr(x), K, M, N, K, L.ptr(ws), nb, L.ptr(out), K, _stream()), "m3l_op_gemm_tn (DINO head)")
    return out


TN_OPERAND_LIMIT = 2 ** 31 - 1      # bytes of one operand of m3l_op_gemm_tn (32-bit buffer offsets; include/m3l_amd.h)


def _gemm_tn_rows(dt, y, x, M, N, K):
    """_gemm_tn for a reduction too long for one call: y (M, N) and x (M, K) are cut into chunks of rows whose operands stay below
    TN_OPERAND_LIMIT, the first chunk overwrites `out`, the others add to it, in row order (the same bits on every run)."""
    esize = 2 if dt == DT_BF16 else 4
    if M * max(N, K) * esize < TN_OPERAND_LIMIT:
        return _gemm_tn(dt, y, x, M, N, K)
    rows = (TN_OPERAND_LIMIT - 1) // (max(N, K) * esize) // 64 * 64
    if rows < 64:
        raise L.M3LError(f"gemm_tn: rows of {max(N, K)} elements are too long to cut the {M}-row reduction into chunks below 2 GiB")
    lib = L.lib()
    out = torch.empty(N, K, dtype=torch.float32, device=y.device)
    for m0 in range(0, M, rows):
        mc = min(rows, M - m0)
        nb = lib.m3l_op_gemm_tn_ws_bytes(mc, N, K)
        ws = _ws(nb, y.device)
        L.check(lib.m3l_op_gemm_tn_acc(dt, L.ptr(y[m0:m0 + mc]), N, L.ptr(x[m0:m0 + mc]), K, mc, N, K, L.ptr(ws), nb, L.ptr(out), K, int(m0 > 0), _stream()),
                "m3l_op_gemm_tn_acc (DINO head)")
    return out


def _colsum(dt, y, M, N):
    lib = L.lib()
    out = torch.empty(N, dtype=torch.float32, device=y.device)
    ws = _ws(lib.m3l_op_colsum_ws_bytes(N), y.device)
    L.check(lib.m3l_op_colsum(dt, L.ptr(y), M, N, N, L.ptr(ws), L.ptr(out), _stream()), "m3l_op_colsum (DINO head)")
    return out


class HeadMlpFn(torch.autograd.Function):
    """x (M, in) f32 -> (M, bottleneck) f32 through Linear [+ GELU] ... Linear.  params: weight_0, bias_0, weight_1, ... (bias None when
    the head has none).  Between the layers the activations stay in the compute type; each hidden layer's pre-activation is kept for the
    gelu' epilogue of the input-gradient GEMM of the layer above it."""

    @staticmethod
    def forward(ctx, dt, x, *params):
        _require_cuda(x, "DINO head input")
        x = _f32c(x)
        M = x.shape[0]
        ws_, bs_ = [_f32c(p) for p in params[0::2]], [_f32c(p) for p in params[1::2]]
        n = len(ws_)
        h, hs, us = _cast(x, dt), [], []
        y = None
        for i, (w, b) in enumerate(zip(ws_, bs_)):
            N, K = w.shape
            hs.append(h)
            wt = _cast(w, dt)
            if i < n - 1:
                a = torch.empty(M, N, dtype=tdtype(dt), device=x.device)
                u = torch.empty_like(a)
                _gemm_nt(dt, h, wt, M, N, K, bias=b, out_t=a, out_pre=u, act=1)
                us.append(u)
                h = a
            else:
                y = torch.empty(M, N, dtype=torch.float32, device=x.device)
                _gemm_nt(dt, h, wt, M, N, K, bias=b, out_f32=y)
        ctx.saved = (dt, M, ws_, [b is not None for b in bs_], hs, us)
        return y

    @staticmethod
    def backward(ctx, dy):
        dt, M, ws_, has_b, hs, us = ctx.saved
        d = _cast(_f32c(dy), dt)
        grads = [None] * (2 * len(ws_))
        dx = None
        for i in range(len(ws_) - 1, -1, -1):
            N, K = ws_[i].shape
            grads[2 * i] = _gemm_tn(dt, d, hs[i], M, N, K)
            if has_b[i]:
                grads[2 * i + 1] = _colsum(dt, d, M, N)
            if i > 0:
                prev = torch.empty(M, K, dtype=tdtype(dt), device=d.device)
                _gemm_nt(dt, d, _cast(ws_[i], dt, transposed=True), M, K, N, out_t=prev, gelu_u=us[i - 1])
                d = prev
            elif ctx.needs_input_grad[1]:
                dx = torch.empty(M, K, dtype=torch.float32, device=d.device)
                _gemm_nt(dt, d, _cast(ws_[i], dt, transposed=True), M, K, N, out_f32=dx)
        return (None, dx) + tuple(grads)


class L2NormFn(torch.autograd.Function):
    """F.normalize(x, dim=-1, p=2, eps) for x (M, D) f32."""

    @staticmethod
    def forward(ctx, x, eps):
        _require_cuda(x, "l2norm input")
        x = _f32c(x)
        M, D = x.shape
        y = torch.empty_like(x)
        norm = torch.empty(M, dtype=torch.float32, device=x.device)
        L.check(L.lib().m3l_op_l2norm_fwd(DT_F32, L.ptr(x), M, D, float(eps), None, L.ptr(y), L.ptr(norm), _stream()), "m3l_op_l2norm_fwd")
        ctx.saved = (x, norm, float(eps))
        return y

    @staticmethod
    def backward(ctx, dy):
        x, norm, eps = ctx.saved
        M, D = x.shape
        dx = torch.empty_like(x)
        L.check(L.lib().m3l_op_l2norm_bwd(L.ptr(_f32c(dy)), L.ptr(x), L.ptr(norm), M, D, eps, L.ptr(dx), _stream()), "m3l_op_l2norm_bwd")
        return dx, None


def _weightnorm(dt, v, g):
    """v (K, D), g (K, 1) -> W (K, D) in the compute type and ||v[k]||."""
    K, D = v.shape
    w = torch.empty(K, D, dtype=tdtype(dt), device=v.device)
    vnorm = torch.empty(K, dtype=torch.float32, device=v.device)
    L.check(L.lib().m3l_op_weightnorm_fwd(dt, L.ptr(v), L.ptr(g), K, D, L.ptr(w), L.ptr(vnorm), _stream()), "m3l_op_weightnorm_fwd")
    return w, vnorm


def _pad_rows(x, rows):
    """(M, n) -> (rows, n) with zero rows appended (the GEMMs want leading dimensions that are multiples of 8)."""
    if x.shape[0] == rows:
        return x
    out = torch.zeros(rows, x.shape[1], dtype=x.dtype, device=x.device)
    out[:x.shape[0]] = x
    return out


def _ld8(rows):
    return (rows + 7) // 8 * 8


def _last_layer_backward(dt, dST, xn, w, v, g, vnorm, need_dx):
    """dS^T (K, ldr) in the compute type, x_n (M, D) f32, W (K, D) -> dx_n (M, D) f32, dv, dg.  Both products have K (the prototypes) as
    their long side: dW = dS^T x_n is an NT GEMM with K rows, dx_n = dS W a TN GEMM that reduces over K in splits; then the weight-norm
    backward."""
    K, D = v.shape
    M, ldr = xn.shape[0], dST.shape[1]
    xnT = _cast(_pad_rows(xn, ldr), dt, transposed=True)              # (D, ldr)
    dW = torch.empty(K, D, dtype=torch.float32, device=dST.device)
    _gemm_nt(dt, dST, xnT, K, D, ldr, out_f32=dW)
    dx = _gemm_tn_rows(dt, dST, w, K, ldr, D)[:M] if need_dx else None
    dv, dg = torch.empty_like(v), torch.empty_like(g)
    L.check(L.lib().m3l_op_weightnorm_bwd(L.ptr(dW), L.ptr(v), L.ptr(g), L.ptr(vnorm), K, D, L.ptr(dv), L.ptr(dg), _stream()), "m3l_op_weightnorm_bwd")
    return dx, dv, dg


class WeightNormLinearFn(torch.autograd.Function):
    """logits (M, K) f32 = x_n W^T, W = weight_norm(v, g): the prototype layer on its own (teacher pass, head used outside the fused loss)."""

    @staticmethod
    def forward(ctx, dt, xn, v, g):
        _require_cuda(xn, "DINO head input")
        xn, v, g = _f32c(xn), _f32c(v), _f32c(g)
        M, D = xn.shape
        K = v.shape[0]
        w, vnorm = _weightnorm(dt, v, g)
        y = torch.empty(M, K, dtype=torch.float32, device=xn.device)
        _gemm_nt(dt, _cast(xn, dt), w, M, K, D, out_f32=y)
        ctx.saved = (dt, xn, w, v, g, vnorm)
        return y

    @staticmethod
    def backward(ctx, dy):
        dt, xn, w, v, g, vnorm = ctx.saved
        dST = _cast(_pad_rows(_f32c(dy), _ld8(xn.shape[0])), dt, transposed=True)
        dx, dv, dg = _last_layer_backward(dt, dST, xn, w, v, g, vnorm, ctx.needs_input_grad[1])
        return None, dx, dv, dg


def _row_stats(logits, rows, K, center, inv_temp):
    lib = L.lib()
    stats = torch.empty(rows, 2, dtype=torch.float32, device=logits.device)
    ws = _ws(lib.m3l_op_dino_ws_bytes(rows, K), logits.device)
    L.check(lib.m3l_op_dino_rowstats(L.ptr(logits), rows, K, L.ptr(center), float(inv_temp), L.ptr(ws), L.ptr(stats), _stream()), "m3l_op_dino_rowstats")
    return stats


def _gather_col_pairs(pairs, group=None):
    """(K, 2) column pairs of this rank -> (world, K, 2), every rank's in rank order (the same tensor on every rank).  Device-agnostic."""
    world = dist.get_world_size(group)
    out = torch.empty((world,) + tuple(pairs.shape), dtype=pairs.dtype, device=pairs.device)
    dist.all_gather(list(out.unbind(0)), pairs.contiguous(), group=group)
    return out


def _probs(logits, rows, K, center, inv_temp, stats):
    out = torch.empty(rows, K, dtype=torch.float32, device=logits.device)
    L.check(L.lib().m3l_op_sk_probs(L.ptr(logits), rows, K, L.ptr(center), float(inv_temp), L.ptr(stats), L.ptr(out), _stream()), "m3l_op_sk_probs")
    return out


def _teacher_rows(teacher_output):
    _require_cuda(teacher_output, "teacher logits")
    T = _f32c(teacher_output)
    K = T.shape[-1]
    return T.reshape(-1, K), T.numel() // K, K


IBOT_MAX_ROWS = 65535          # Q R of one call (include/m3l_amd.h, "iBOT patch loss")


def _patch_rows_check(P, Q, rows):
    if P != Q:
        raise ValueError(f"iBOT patch loss: as many student as teacher views expected, got {P} and {Q}")
    if Q * rows > IBOT_MAX_ROWS:
        raise ValueError(f"iBOT patch loss: {Q} x {rows} patch rows in one call, at most {IBOT_MAX_ROWS}")


class RowFamily(NamedTuple):
    """One kernel family of the paired-row cross-entropy: student views (P, rows, K) against teacher views (Q, rows, K), row r of every student
    view paired with row r of every teacher view.  `c_loss` and `c_grad` take (lib, S, T, center, P, Q, rows, K, inv_ts, inv_tt, ...) and put
    the arguments into their C function's order, nothing more; `check` raises for a shape the family cannot run.  The caller names the
    family: it is never chosen from the shape."""
    name: str           # m3l_op_<name>_loss / _grad in error messages
    ws_bytes: Callable  # (lib, rows, K) -> bytes of the loss kernel's workspace
    c_loss: Callable
    c_grad: Callable
    check: Callable     # (P, Q, rows)
    keep: str           # key under which the head + loss node leaves the student logits in `keep`

    def args(self, student, teacher, center):
        _require_cuda(student, "student logits")
        S, T = _f32c(student), _f32c(teacher)
        if S.dim() != 3 or T.dim() != 3 or S.shape[1:] != T.shape[1:]:
            raise ValueError(f"student (P, rows, K) and teacher (Q, rows, K) logits expected, got {tuple(S.shape)} and {tuple(T.shape)}")
        self.check(S.shape[0], T.shape[0], S.shape[1])
        c = _f32c(center).reshape(-1)
        if c.numel() != S.shape[2]:
            raise ValueError(f"center has {c.numel()} entries for K = {S.shape[2]}")
        return S, T, c

    def loss_forward(self, S, T, center, P, Q, rows, K, inv_ts, inv_tt):
        lib = L.lib()
        s_stats = _row_stats(S, P * rows, K, None, inv_ts)
        t_stats = _row_stats(T, Q * rows, K, center, inv_tt)
        loss = torch.empty((), dtype=torch.float32, device=S.device)
        ws = _ws(self.ws_bytes(lib, rows, K), S.device)
        L.check(self.c_loss(lib, L.ptr(S), L.ptr(T), L.ptr(center), P, Q, rows, K, inv_ts, inv_tt, L.ptr(s_stats), L.ptr(t_stats), L.ptr(ws),
                            L.ptr(loss), _stream()), f"m3l_op_{self.name}_loss")
        return loss, s_stats, t_stats

    def loss_grad(self, dt, S, T, center, P, Q, rows, K, inv_ts, inv_tt, s_stats, t_stats, dloss):
        """-> dS^T (K, ldr) in the compute type, ldr = P rows rounded up to a multiple of 8 (pad columns zero)."""
        ldr = _ld8(P * rows)
        dST = torch.empty(K, ldr, dtype=tdtype(dt), device=S.device)
        L.check(self.c_grad(L.lib(), dt, L.ptr(S), L.ptr(T), L.ptr(center), P, Q, rows, K, inv_ts, inv_tt, L.ptr(s_stats), L.ptr(t_stats),
                            L.ptr(dloss), L.ptr(dST), ldr, _stream()), f"m3l_op_{self.name}_grad")
        return dST


# m3l_op_dino_*: the teacher sums of a sample stay in LDS, any P and Q, rows <= 255 (checked in C)
DINO_ROWS = RowFamily("dino", lambda lib, rows, K: lib.m3l_op_dino_ws_bytes(rows, K),
                      lambda lib, S, T, c, P, Q, rows, K, *tail: lib.m3l_op_dino_loss(S, P, T, Q, rows, K, c, *tail),
                      lambda lib, dt, S, T, c, P, Q, rows, K, *tail: lib.m3l_op_dino_grad(dt, S, P, T, Q, rows, K, c, *tail),
                      lambda P, Q, rows: None, "student_logits")
# m3l_op_ibot_*: tiles over the rows, P = Q, Q rows <= IBOT_MAX_ROWS
PATCH_ROWS = RowFamily("ibot", lambda lib, rows, K: lib.m3l_op_ibot_ws_bytes(rows, K),
                       lambda lib, S, T, c, P, Q, rows, K, *tail: lib.m3l_op_ibot_loss(S, T, Q, rows, K, c, *tail),
                       lambda lib, dt, S, T, c, P, Q, rows, K, *tail: lib.m3l_op_ibot_grad(dt, S, T, Q, rows, K, c, *tail),
                       _patch_rows_check, "student_patch_logits")

# one family's helpers under the names and argument lists they had while each family had helpers of its own; the kernel tests call these
_loss_forward, _loss_grad = DINO_ROWS.loss_forward, DINO_ROWS.loss_grad


def _ibot_grad(dt, S, T, center, Q, *rest):
    return PATCH_ROWS.loss_grad(dt, S, T, center, Q, Q, *rest)


class RowLossFn(torch.autograd.Function):
    """loss(student (P, rows, K), teacher logits (Q, rows, K), center (K)) with an f32 gradient for the student logits: the loss on its own.
    A subclass sets `family`, nothing else."""
    family = None

    @staticmethod
    def forward(ctx, student, teacher, center, student_temp, teacher_temp):
        family = ctx._forward_cls.family
        S, T, c = family.args(student, teacher, center)
        (P, rows, K), Q = S.shape, T.shape[0]
        inv_ts, inv_tt = 1.0 / float(student_temp), 1.0 / float(teacher_temp)
        loss, s_stats, t_stats = family.loss_forward(S, T, c, P, Q, rows, K, inv_ts, inv_tt)
        ctx.saved = (S, T, c.clone(), P, Q, rows, K, inv_ts, inv_tt, s_stats, t_stats)
        return loss

    @staticmethod
    def backward(ctx, dloss):
        S, T, c, P, Q, rows, K, inv_ts, inv_tt, s_stats, t_stats = ctx.saved
        dST = ctx._forward_cls.family.loss_grad(DT_F32, S, T, c, P, Q, rows, K, inv_ts, inv_tt, s_stats, t_stats, _f32c(dloss))
        return dST.t()[:P * rows].reshape(P, rows, K), None, None, None, None


class RowHeadLossFn(torch.autograd.Function):
    """Prototype layer + loss in one node: x_n (P rows, D) f32, v, g, teacher logits (Q, rows, K), center -> loss.  The gradient kernel writes
    dS^T in the compute type, which is what the two backward GEMMs of the prototype layer read; no f32 (P rows, K) gradient exists.
    A subclass sets `family`, nothing else."""
    family = None

    @staticmethod
    def forward(ctx, dt, P, xn, v, g, teacher, center, student_temp, teacher_temp, keep):
        family = ctx._forward_cls.family
        _require_cuda(xn, "DINO head input")
        xn, v, g = _f32c(xn), _f32c(v), _f32c(g)
        M, D = xn.shape
        K, rows = v.shape[0], M // P
        w, vnorm = _weightnorm(dt, v, g)
        S = torch.empty(P, rows, K, dtype=torch.float32, device=xn.device)
        _gemm_nt(dt, _cast(xn, dt), w, M, K, D, out_f32=S)
        S, T, c = family.args(S, teacher, center)
        Q = T.shape[0]
        inv_ts, inv_tt = 1.0 / float(student_temp), 1.0 / float(teacher_temp)
        loss, s_stats, t_stats = family.loss_forward(S, T, c, P, Q, rows, K, inv_ts, inv_tt)
        ctx.saved = (dt, xn, w, v, g, vnorm, S, T, c.clone(), P, Q, rows, K, inv_ts, inv_tt, s_stats, t_stats)
        if keep is not None:
            keep[family.keep] = S
        return loss

    @staticmethod
    def backward(ctx, dloss):
        dt, xn, w, v, g, vnorm, S, T, c, P, Q, rows, K, inv_ts, inv_tt, s_stats, t_stats = ctx.saved
        dST = ctx._forward_cls.family.loss_grad(dt, S, T, c, P, Q, rows, K, inv_ts, inv_tt, s_stats, t_stats, _f32c(dloss))
        dx, dv, dg = _last_layer_backward(dt, dST, xn, w, v, g, vnorm, ctx.needs_input_grad[2])
        return None, None, dx, dv, dg, None, None, None, None, None


class DinoLossFn(RowLossFn):
    family = DINO_ROWS


class IbotLossFn(RowLossFn):
    family = PATCH_ROWS


class HeadLossFn(RowHeadLossFn):
    family = DINO_ROWS


class IbotHeadLossFn(RowHeadLossFn):
    family = PATCH_ROWS


class WeightNormLinear(nn.Module):
    """`weight_norm(nn.Linear(in, out, bias=False))`: parameters weight_g (out, 1) and weight_v (out, in), registered in that order; weight_v
    gets nn.Linear's default initial values, weight_g the row norms."""

    def __init__(self, in_features, out_features):
        super().__init__()
        self.in_features, self.out_features = in_features, out_features
        v = torch.empty(out_features, in_features)
        nn.init.kaiming_uniform_(v, a=math.sqrt(5))
        self.weight_g = nn.Parameter(v.norm(dim=1, keepdim=True))
        self.weight_v = nn.Parameter(v)


class DINOHead(nn.Module):
    def __init__(self, in_dim, out_dim, use_bn=False, nlayers=3, hidden_dim=2048, bottleneck_dim=256, mlp_bias=True, compute_dtype="fp32"):
        super().__init__()
        if use_bn:
            raise NotImplementedError("DINOHead(use_bn=True): BatchNorm1d between the head's layers has no kernel here; no configuration of "
                                      "the reference sets it")
        nlayers = max(nlayers, 1)
        if nlayers == 1:
            self.mlp = nn.Linear(in_dim, bottleneck_dim, bias=mlp_bias)
        else:
            layers = [nn.Linear(in_dim, hidden_dim, bias=mlp_bias), nn.GELU()]
            for _ in range(nlayers - 2):
                layers += [nn.Linear(hidden_dim, hidden_dim, bias=mlp_bias), nn.GELU()]
            layers.append(nn.Linear(hidden_dim, bottleneck_dim, bias=mlp_bias))
            self.mlp = nn.Sequential(*layers)
        for m in self.modules():
            if isinstance(m, nn.Linear):
                trunc_normal_(m.weight, std=0.02)
                if m.bias is not None:
                    nn.init.constant_(m.bias, 0)
        self.last_layer = WeightNormLinear(bottleneck_dim, out_dim)
        self.last_layer.weight_g.data.fill_(1)
        self.compute_dtype = compute_dtype
        self.eps = 1e-12

    def _linears(self):
        return [self.mlp] if isinstance(self.mlp, nn.Linear) else [m for m in self.mlp if isinstance(m, nn.Linear)]

    def normalized(self, x):
        """(..., in_dim) -> (rows, bottleneck) L2-normalised bottleneck vectors."""
        dt = dtype_code(self.compute_dtype)
        params = []
        for lin in self._linears():
            params += [lin.weight, lin.bias]
        y = HeadMlpFn.apply(dt, x.reshape(-1, x.shape[-1]), *params)
        return L2NormFn.apply(y, self.eps)

    def forward(self, x):
        xn = self.normalized(x)
        y = WeightNormLinearFn.apply(dtype_code(self.compute_dtype), xn, self.last_layer.weight_v, self.last_layer.weight_g)
        return y.view(*x.shape[:-1], y.shape[-1])


@torch.no_grad()
def _sinkhorn_knopp_center(teacher_logits, teacher_temp, n_iterations, process_group):
    """The (K,) float32 vector c with sinkhorn_knopp_teacher(T) = softmax((T - c) / teacher_temp): `n_iterations` column passes over the
    rows of every rank (each rank's pairs all-gathered over `process_group` and merged in rank order) and n_iterations - 1 local row
    passes.  Pass it where the loss functions take the centre."""
    if n_iterations < 1:
        raise ValueError(f"sinkhorn_knopp: n_iterations = {n_iterations}; without a column normalisation the result is no distribution")
    T, rows, K = _teacher_rows(teacher_logits)
    lib = L.lib()
    temp, inv_temp = float(teacher_temp), 1.0 / float(teacher_temp)
    center = torch.empty(K, dtype=torch.float32, device=T.device)
    pairs = torch.empty(K, 2, dtype=torch.float32, device=T.device)
    ws = _ws(lib.m3l_op_sk_ws_bytes(rows, K), T.device)
    stats = None
    for it in range(n_iterations):
        L.check(lib.m3l_op_sk_colstats(L.ptr(T), rows, K, inv_temp, L.ptr(stats), L.ptr(ws), L.ptr(pairs), _stream()), "m3l_op_sk_colstats")
        parts = _gather_col_pairs(pairs, process_group) if dist.is_initialized() else pairs
        L.check(lib.m3l_op_sk_colcombine(L.ptr(parts), parts.numel() // (2 * K), K, temp, L.ptr(center), _stream()), "m3l_op_sk_colcombine")
        if it < n_iterations - 1:
            stats = _row_stats(T, rows, K, center, inv_temp)
    return center


class CenteredLoss(nn.Module):
    """What DINOLoss and iBOTPatchLoss share: the centre with its one-step delay, the two target distributions and `forward`.

    `forward(student (P, rows, K), teacher logits (Q, rows, K), teacher_temp)` applies the pending centre update, computes the loss against the
    centred teacher through `loss_fn` and leaves this step's teacher column sums pending (as the reference's softmax_center_teacher /
    update_center pair).  With torch.distributed initialised the pending sums are all-reduced asynchronously over `process_group` and divided by
    count x world size; on one rank they are the local sums.  `forward(..., centering="sinkhorn_knopp")` takes the Sinkhorn-Knopp targets
    instead and leaves the centre alone; `softmax_center_teacher` / `sinkhorn_knopp_teacher` return the two target distributions themselves,
    as the reference's methods of those names do.

    A subclass sets `loss_fn` (the loss node of its kernel family) and `count_name` (the reference's attribute for the count the pending
    sums are divided by) and gives `_center_sum(T, rows, K, out)`, which launches its column sums of T into `out` and returns that count."""
    loss_fn = count_name = None

    def __init__(self, center_shape, student_temp, center_momentum, process_group):
        super().__init__()
        self.student_temp = student_temp
        self.center_momentum = center_momentum
        self.register_buffer("center", torch.zeros(center_shape))
        self.process_group = process_group
        self.updated = True
        self.reduce_handle = None
        setattr(self, self.count_name, None)
        self.async_batch_center = None

    @torch.no_grad()
    def apply_center_update(self):
        if self.updated is False:
            world = dist.get_world_size(self.process_group) if dist.is_initialized() else 1
            if self.reduce_handle is not None:
                self.reduce_handle.wait()
                self.reduce_handle = None
            K = self.center.shape[-1]
            if self.center.dtype != torch.float32 or not self.center.is_contiguous():
                raise L.M3LError(f"{type(self).__name__}.center must be a contiguous float32 buffer")
            m, count = float(self.center_momentum), float(getattr(self, self.count_name) * world)
            L.check(L.lib().m3l_op_dino_center_apply(L.ptr(self.center), L.ptr(self.async_batch_center), K, m, 1 - m, count, _stream()), "m3l_op_dino_center_apply")
            self.updated = True

    @torch.no_grad()
    def update_center(self, teacher_output):
        _require_cuda(teacher_output, "teacher logits")
        T = _f32c(teacher_output)
        K = T.shape[-1]
        pending = torch.empty(1, K, dtype=torch.float32, device=T.device)
        count = self._center_sum(T, T.numel() // K, K, pending)
        self.updated = False
        setattr(self, self.count_name, count)
        self.async_batch_center = pending
        if dist.is_initialized():
            self.reduce_handle = dist.all_reduce(self.async_batch_center, op=dist.ReduceOp.SUM, group=self.process_group, async_op=True)

    def sinkhorn_knopp_center(self, teacher_logits, teacher_temp, n_iterations=3):
        """The (K,) float32 vector c with sinkhorn_knopp_teacher(T) = softmax((T - c) / teacher_temp), over `process_group` (_sinkhorn_knopp_center)."""
        return _sinkhorn_knopp_center(teacher_logits, teacher_temp, n_iterations, self.process_group)

    def _targets(self, teacher_output, teacher_temp, center):
        T, rows, K = _teacher_rows(teacher_output)
        inv_temp = 1.0 / float(teacher_temp)
        return _probs(T, rows, K, center, inv_temp, _row_stats(T, rows, K, center, inv_temp))

    @torch.no_grad()
    def sinkhorn_knopp_teacher(self, teacher_output, teacher_temp, n_iterations=3):
        """The reference's return value: the assignment as probabilities, (rows, K) float32 with the leading dimensions flattened to rows."""
        return self._targets(teacher_output, teacher_temp, self.sinkhorn_knopp_center(teacher_output, teacher_temp, n_iterations))

    @torch.no_grad()
    def softmax_center_teacher(self, teacher_output, teacher_temp):
        """softmax((teacher_output - center) / teacher_temp) after the pending centre update, (rows, K) float32."""
        self.apply_center_update()
        return self._targets(teacher_output, teacher_temp, _f32c(self.center).reshape(-1))

    def forward(self, student_logits, teacher_logits, teacher_temp, centering="centering", n_iterations=3):
        if centering == "sinkhorn_knopp":
            # the centre, `updated` and the pending sums stay as they are: this branch of the reference never calls update_center
            center = self.sinkhorn_knopp_center(teacher_logits, teacher_temp, n_iterations)
            return self.loss_fn.apply(student_logits, teacher_logits, center, self.student_temp, teacher_temp)
        if centering != "centering":
            raise ValueError(f"{type(self).__name__}.forward: centering must be 'centering' or 'sinkhorn_knopp', got {centering!r}")
        self.apply_center_update()
        loss = self.loss_fn.apply(student_logits, teacher_logits, self.center, self.student_temp, teacher_temp)
        self.update_center(teacher_logits)
        return loss


class DINOLoss(CenteredLoss):
    """The DINO loss with its centre, buffer `center` (1, K): CenteredLoss over student (P, B, K) and teacher (Q, B, K) logits on the kernels
    that keep a sample's teacher sums in LDS (m3l_op_dino_*).  The pending sums are the plain column sums, `len_teacher_output` their rows."""
    loss_fn, count_name = DinoLossFn, "len_teacher_output"

    def __init__(self, out_dim, student_temp=0.1, center_momentum=0.9, process_group=None):
        super().__init__((1, out_dim), student_temp, center_momentum, process_group)

    def _load_from_state_dict(self, state_dict, prefix, *args, **kwargs):
        # the reference's centre becomes (1, 1, K) at its first update (it broadcasts against the (rows, 1, K) teacher output): same values
        c = state_dict.get(prefix + "center")
        if c is not None and c.dim() == 3 and c.shape[0] == 1 and tuple(c.shape[1:]) == tuple(self.center.shape):
            state_dict[prefix + "center"] = c[0]
        super()._load_from_state_dict(state_dict, prefix, *args, **kwargs)

    def _center_sum(self, T, rows, K, out):
        L.check(L.lib().m3l_op_dino_center_sum(L.ptr(T), rows, K, L.ptr(out), _stream()), "m3l_op_dino_center_sum")
        return rows


class KoLeoFn(torch.autograd.Function):
    """KoLeo loss of x (groups * n, D) f32, summed over `groups` independent sets of n consecutive rows -> 0-d f32.  keep["indices"] receives
    the (groups, n) int64 nearest neighbours (index inside the group).  The neighbours are constants for the gradient."""

    @staticmethod
    def forward(ctx, x, groups, eps, keep):
        _require_cuda(x, "KoLeo input")
        x = _f32c(x)
        if x.dim() != 2 or groups < 1 or x.shape[0] % groups:
            raise ValueError(f"KoLeoFn: (groups * n, D) rows expected, got {tuple(x.shape)} for {groups} group(s)")
        lib = L.lib()
        (M, D), n = x.shape, x.shape[0] // groups
        y = torch.empty_like(x)
        norm = torch.empty(M, dtype=torch.float32, device=x.device)
        dist_ = torch.empty(M, dtype=torch.float32, device=x.device)
        nn32 = torch.empty(M, dtype=torch.int32, device=x.device)
        nn64 = torch.empty(groups, n, dtype=torch.int64, device=x.device)
        loss = torch.empty((), dtype=torch.float32, device=x.device)
        ws = _ws(lib.m3l_op_koleo_ws_bytes(groups, n, D), x.device)
        L.check(lib.m3l_op_koleo_fwd(L.ptr(x), groups, n, D, float(eps), L.ptr(ws), L.ptr(y), L.ptr(norm), L.ptr(nn32), L.ptr(nn64), L.ptr(dist_),
                                     L.ptr(loss), _stream()), "m3l_op_koleo_fwd")
        ctx.saved = (x, y, norm, nn32, dist_, groups, n, D, float(eps))
        if keep is not None:
            keep["indices"] = nn64
        return loss

    @staticmethod
    def backward(ctx, dloss):
        x, y, norm, nn32, dist_, groups, n, D, eps = ctx.saved
        dx = torch.empty_like(x)
        L.check(L.lib().m3l_op_koleo_bwd(L.ptr(_f32c(dloss)), L.ptr(x), L.ptr(y), L.ptr(norm), L.ptr(nn32), L.ptr(dist_), groups, n, D, eps, L.ptr(dx),
                                         _stream()), "m3l_op_koleo_bwd")
        return dx, None, None, None


class KoLeoLoss(nn.Module):
    """Kozachenko-Leonenko regulariser (`tactile_ssl/loss/koleo_loss.py`): -mean_i log(||y_i - y_I(i) + 1e-8|| + eps) over the L2-normalised
    rows y of a (B, D) batch, I(i) the row with the largest inner product with row i.  No parameters, no buffers; float32 whatever the
    model's compute type (the reference switches autocast off).  `last` holds the neighbours of the last call."""

    def __init__(self):
        super().__init__()
        self.last = None

    @torch.no_grad()
    def pairwise_NNs_inner(self, x):
        """(B,) int64 nearest neighbours of the rows of x by inner product (the kernel normalises; a normalised x is left as it is up to
        rounding, and the neighbours of x and of normalize(x) are the same rows)."""
        keep = {}
        KoLeoFn.apply(x.detach(), 1, 1e-8, keep)
        return keep["indices"][0]

    def forward(self, student_output, eps=1e-8):
        keep = {}
        loss = KoLeoFn.apply(student_output, 1, eps, keep)
        self.last = keep["indices"][0]
        return loss


def _stack_views(x):
    return torch.stack(list(x)) if isinstance(x, (list, tuple)) else x


class iBOTPatchLoss(CenteredLoss):
    """The reference's iBOTPatchLoss (`tactile_ssl/loss/ibot_patch_loss.py`) on the row-tiled kernels (m3l_op_ibot_*): buffer `center` (1, 1, K).

    `forward(student_logits, teacher_logits, teacher_temp)` takes the LOGITS of Q student and Q teacher views, (Q, R, K) tensors or lists of Q
    (R, K) tensors with R = B n patch rows (row r of every student view is paired with row r of every teacher view), and returns the
    reference's unscaled `forward`: sum over all (student view, teacher view) pairs of the mean over rows of the cross-entropy.  The centre
    is CenteredLoss's, as DINOLoss's: the pending update is applied first, this step's sums are left pending (one-step delay) and are
    all-reduced asynchronously over `process_group`.  `update_center` takes the reference's (Q B, n, K) teacher tokens: pending = sum_b mean_k,
    count = Q B x world; handed (Q, R, K), as `forward` is, it takes the Q views as the samples (pending = sum over rows / R, count = Q), which
    is the same centre.  `centering="sinkhorn_knopp"` takes the Sinkhorn-Knopp targets over all Q R rows and leaves the centre alone.

    `sinkhorn_knopp_teacher(teacher_output, teacher_temp, n_masked_patches_tensor)`: the reference divides by B = n_masked_patches_tensor after
    each column normalisation, the next normalisation removes any constant factor, and its final `Q *= B` restores the last one, so the
    argument does not change the result; it is accepted and ignored (tests/golden/ibot_loss.npz pins this with two values).

    Not built: `forward_masked` (nothing in the reference calls it)."""
    loss_fn, count_name = IbotLossFn, "len_teacher_patch_tokens"

    def __init__(self, patch_out_dim, student_temp=0.1, center_momentum=0.9, process_group=None):
        super().__init__((1, 1, patch_out_dim), student_temp, center_momentum, process_group)

    def _center_sum(self, T, rows, K, out):
        if T.dim() < 3:
            raise ValueError(f"iBOTPatchLoss.update_center: (samples, patches, K) teacher logits expected, got {tuple(T.shape)}")
        lib = L.lib()
        samples = T.shape[0]
        ws = _ws(lib.m3l_op_ibot_ws_bytes(rows, K), T.device)
        L.check(lib.m3l_op_ibot_center_sum(L.ptr(T), rows, K, float(samples) / float(rows), L.ptr(ws), L.ptr(out), _stream()), "m3l_op_ibot_center_sum")
        return samples

    reduce_center_update = CenteredLoss.update_center

    @torch.no_grad()
    def sinkhorn_knopp_teacher(self, teacher_output, teacher_temp, n_masked_patches_tensor=None, n_iterations=3):
        """(rows, K) float32 probabilities.  `n_masked_patches_tensor` cancels (class docstring) and is ignored."""
        return super().sinkhorn_knopp_teacher(teacher_output, teacher_temp, n_iterations)

    @torch.no_grad()
    def softmax_center_teacher(self, teacher_patch_tokens, teacher_temp):
        """softmax((teacher_patch_tokens - center) / teacher_temp) after the pending centre update, float32 in the shape of the input."""
        return super().softmax_center_teacher(teacher_patch_tokens, teacher_temp).view(teacher_patch_tokens.shape)

    def forward(self, student_logits, teacher_logits, teacher_temp, centering="centering", n_iterations=3):
        return super().forward(_stack_views(student_logits), _stack_views(teacher_logits), teacher_temp, centering, n_iterations)


@torch.no_grad()
def update_moving_average(ma_model, current_model, beta):
    """teacher_p = teacher_p * beta + (1 - beta) * student_p over the two modules' parameters() paired in order, in one multi-tensor launch."""
    dst, src = [], []
    for cur, ma in zip(current_model.parameters(), ma_model.parameters()):
        if cur.shape != ma.shape:
            raise ValueError(f"moving average over parameters of different shapes: {tuple(ma.shape)} and {tuple(cur.shape)}")
        _require_cuda(ma, "moving-average parameter")
        if ma.dtype != torch.float32 or cur.dtype != torch.float32 or not ma.is_contiguous() or not cur.is_contiguous():
            raise L.M3LError("update_moving_average needs contiguous float32 parameters")
        if ma.numel():
            dst.append(ma)
            src.append(cur)
    if not dst:
        return
    n = len(dst)
    lens = (C.c_long * n)(*[t.numel() for t in dst])
    beta = float(beta)
    L.check(L.lib().m3l_op_ema(L.ptr_array(dst), L.ptr_array(src), lens, n, beta, 1.0 - beta, _stream()), "m3l_op_ema")
