"""The SAC head with an ensemble of N critics on the HIP kernels of m3l_amd/csrc/sac.hip ("SAC critic ensemble" of include/m3l_amd.h): what a
high update-to-data ratio needs (REDQ, Chen et al. 2021: N critics, the target's minimum over a random subset of M of them, the actor trained
against the ensemble's mean), and SB3's `n_critics` of any value, which `MAESACPolicy` passes on (`sac_mae_policy.py:62`).

  rule  : q_c = critic_c(cat([x, a])) per critic as in `m3l_amd.sac`;
          target_q = r + (1 - done) * gamma * (min over `subset` of q_target_c(x', a') - ent_coef * logp');
          critic_loss = 0.5 * sum_c mean(weights * (q_c - target_q)^2) (SB3's sum over the critics), td = mean_c |q_c - target_q|;
          actor_loss = mean(ent_coef * logp - min_c q_c) (q_reduce="min", SB3's) or mean(ent_coef * logp - mean_c q_c) (q_reduce="mean", REDQ's).
  nodes : the actor's are `m3l_amd.sac`'s (`SACActorFn`, the entropy-coefficient loss); `SACEnsCriticFn` (1 launch forward; backward 1 chain
          launch + ceil(N * (layers per critic) / 8) weight-gradient launches) and one node per loss (1 + 1).  `td_target` is one launch without a
          tape, and evaluates only the critics of `subset`.  Nothing is read back to the host: the subset is drawn and stays on the device.

Neither SB3 nor a REDQ implementation is part of the reference tree: PARITY UNPINNED; tests/sac_ens_cases.py restates the rule in float64.
`SACHead` and its refusal of any `n_critics` but 2 are unchanged; with N = 2, subset=None and q_reduce="min" the losses here have its bits.
TQC (quantile critics) is `m3l_amd.tqc.TQCHead`.  Everything is float32; there is no eager fallback.

DroQ critics (include/m3l_amd.h "SAC DroQ critics", Hiraoka et al. 2022): `SACEnsembleHead(critic_layer_norm=True, critic_dropout=p)` gives every
critic and target critic hidden layers Linear -> Dropout(p) -> LayerNorm -> ReLU, and `q_values` / `td_target` then run the m3l_sac_droq_*
entries (`SACDroqCriticFn`: the ensemble's launches plus one for every d gamma / d beta).  Masks come from the Philox contract of the
transformer's dropout, one 63-bit seed per call from torch's CPU generator (or `dropout_seed=`), and are regenerated in the backward, never
stored.  The losses, the subset logic and `polyak_update` are the ensemble's.  PARITY UNPINNED; tests/droq_cases.py restates the rule in float64."""
import ctypes as C
import numbers
from typing import NamedTuple, Tuple

import torch
from torch import nn

from . import _head as H
from . import _lib as L
from . import sac as S
from ._head import _dev, _vec
from .dino import update_moving_average
from .functional import _require_cuda, _stream, _ws
from .sac import MAX_CRITICS, WB

Q_REDUCE = {"min": 0, "mean": 1}


def _n_critics_of(n):
    if isinstance(n, bool) or not isinstance(n, numbers.Integral) or not 1 <= n <= MAX_CRITICS:
        raise ValueError(f"n_critics={n!r}: the HIP SAC critic ensemble computes an integer number of critics from 1 to {MAX_CRITICS}")
    return int(n)


def _dropout_of(p):
    """critic_dropout as a float: a real number with 0 <= p < 1."""
    if isinstance(p, bool) or not isinstance(p, numbers.Real) or not 0.0 <= p < 1.0:
        raise ValueError(f"critic_dropout={p!r}: a real number with 0 <= p < 1 expected")
    return float(p)


def _seed_of(seed):
    """A dropout seed as the C ABI takes it: an integer in [0, 2^64)."""
    if isinstance(seed, bool) or not isinstance(seed, numbers.Integral) or not 0 <= seed < 2 ** 64:
        raise ValueError(f"dropout_seed={seed!r}: an integer in [0, 2^64) expected")
    return int(seed)


def draw_seed():
    """A fresh 63-bit seed from torch's default CPU generator, as `Transformer._drop()` draws it: no device sync, `torch.manual_seed` reproduces it."""
    return int(torch.randint(0, 2 ** 63 - 1, (), dtype=torch.int64).item())


class _EnsembleFields(NamedTuple):
    pi: Tuple[WB, ...]
    mu: WB
    log_std: WB
    qf: Tuple[Tuple[WB, ...], ...]
    qf_target: Tuple[Tuple[WB, ...], ...]


class SACEnsembleParams(_EnsembleFields):
    """The parameter tensors of a head with N critics, torch.nn.Linear layouts: `SACHeadParams` with N tuples in qf and in qf_target.  The tuple
    itself stays those five fields; what the DroQ critics add rides along as attributes:
      qf_ln / qf_target_ln   per critic, (weight, bias) of the LayerNorm of every hidden layer; () when the critics have no LayerNorm
      dropout_p              the critics' dropout rate
      drops                  (critic.training, critic_target.training): nn.Dropout's rule, per sub-module"""

    def __new__(cls, pi, mu, log_std, qf, qf_target, qf_ln=(), qf_target_ln=(), dropout_p=0.0, drops=(True, True)):
        self = super().__new__(cls, pi, mu, log_std, qf, qf_target)
        self.qf_ln, self.qf_target_ln, self.dropout_p, self.drops = tuple(qf_ln), tuple(qf_target_ln), float(dropout_p), tuple(drops)
        return self

    @property
    def n_critics(self):
        return len(self.qf)

    @property
    def layer_norm(self):
        return len(self.qf_ln) > 0

    def actor_flat(self):
        return [t for wb in self.pi for t in wb] + list(self.mu) + list(self.log_std)

    def critic_flat(self, target=False):
        return [t for net in (self.qf_target if target else self.qf) for wb in net for t in wb]

    def ln_flat(self, target=False):
        return [t for net in (self.qf_target_ln if target else self.qf_ln) for wb in net for t in wb]

    def active_dropout(self, target=False):
        """The rate the critics (the target critics) drop with in a call made now: p in train mode, 0 in eval mode."""
        return self.dropout_p if self.drops[1 if target else 0] else 0.0

    @staticmethod
    def from_policy(policy) -> "SACEnsembleParams":
        """From a module with SB3's attribute names and `critic.qf0 .. qf{N-1}` (the same for `critic_target`): a `SACEnsembleHead`, or an SB3
        `SACPolicy` with `n_critics` from 1 to 10.  Everything else is checked as `SACHeadParams.from_policy` checks it.  Critics whose hidden
        layers are [Linear, Dropout, LayerNorm, ReLU] (a head built with critic_layer_norm=True) are read as DroQ critics; all critics and
        their targets must then have that layout, one dropout rate, and one train / eval mode per sub-module."""
        S._reject_flags(policy)
        counts = []
        for name, c in (("critic", policy.critic), ("critic_target", policy.critic_target)):
            n = 0
            while hasattr(c, f"qf{n}"):
                n += 1
            told = getattr(c, "n_critics", n)
            if told != n:
                raise ValueError(f"{name}: n_critics={told} but {n} nets qf0 .. are there")
            counts.append(n)
        told = getattr(policy, "n_critics", counts[0])
        if told != counts[0] or counts[1] != counts[0]:
            raise ValueError(f"n_critics={told}, {counts[0]} critics and {counts[1]} target critics: the three must agree")
        n = _n_critics_of(counts[0])
        nets = [(f"{name}.qf{i}", getattr(c, f"qf{i}")) for name, c in (("critic", policy.critic), ("critic_target", policy.critic_target)) for i in range(n)]
        norm = [any(isinstance(m, (nn.LayerNorm, nn.Dropout)) for m in seq) for _, seq in nets]
        told = bool(getattr(policy, "critic_layer_norm", norm[0]))
        if any(v != norm[0] for v in norm) or (norm[0] and not told):
            with_ln = [name for (name, _), v in zip(nets, norm) if v]
            raise ValueError(f"critic_layer_norm={told}, but the nets with LayerNorm / Dropout layers are {with_ln}: all critics and their targets "
                             "must have one layout")
        if not told:
            return SACEnsembleParams(*S._read_policy(policy, n))
        pi, mu, log_std = S._read_policy(_ActorOnly(policy), 0)[:3]
        read = [_droq_net(seq, name) for name, seq in nets]
        rates = {p for _, _, ps, _ in read for p in ps} | ({float(policy.critic_dropout)} if hasattr(policy, "critic_dropout") else set())
        if len(rates) > 1:
            raise ValueError(f"dropout rates {sorted(rates)}: all critics and their targets must have one rate")
        drops = []
        for name, part in (("critic", read[:n]), ("critic_target", read[n:])):
            modes = {t for _, _, _, ts in part for t in ts}
            if len(modes) > 1:
                raise ValueError(f"{name}: some Dropout layers are in train mode and some in eval mode; switch the whole sub-module ({name}.train() / .eval())")
            drops.append(modes.pop() if modes else bool(getattr(getattr(policy, name), "training", True)))
        return SACEnsembleParams(pi, mu, log_std, tuple(r[0] for r in read[:n]), tuple(r[0] for r in read[n:]), tuple(r[1] for r in read[:n]),
                                 tuple(r[1] for r in read[n:]), rates.pop() if rates else 0.0, drops)


class _ActorOnly:
    """The actor's side of a policy for `S._read_policy` with no critics."""

    def __init__(self, policy):
        self.actor, self.critic, self.critic_target = policy.actor, policy.critic, policy.critic_target


def _droq_net(seq, name):
    """((weight, bias) of every Linear, the last being the Linear(., 1)), ((weight, bias) of every LayerNorm), the Dropout rates, their training
    flags, of a net [Linear, Dropout, LayerNorm, ReLU] x n + Linear(., 1)."""
    mods = list(seq)
    if not mods or not isinstance(mods[-1], nn.Linear) or mods[-1].bias is None or mods[-1].out_features != 1:
        raise ValueError(f"{name}: a net ending in nn.Linear(., 1) with a bias expected")
    if (len(mods) - 1) % 4:
        raise ValueError(f"{name}: Linear / Dropout / LayerNorm / ReLU groups and a last Linear expected, got {len(mods)} modules")
    lin, ln, ps, ts = [], [], [], []
    for i in range(0, len(mods) - 1, 4):
        fc, dr, norm, act = mods[i:i + 4]
        if not isinstance(fc, nn.Linear) or fc.bias is None:
            raise ValueError(f"{name}.{i}: nn.Linear with a bias expected, got {type(fc).__name__}")
        if not isinstance(dr, nn.Dropout):
            raise ValueError(f"{name}.{i + 1}: nn.Dropout expected (present at p = 0 too), got {type(dr).__name__}")
        if not isinstance(norm, nn.LayerNorm) or not norm.elementwise_affine or norm.bias is None or tuple(norm.normalized_shape) != (fc.out_features,) \
                or norm.eps != 1e-5:
            raise ValueError(f"{name}.{i + 2}: nn.LayerNorm({fc.out_features}) with an elementwise affine and eps 1e-5 expected, got {norm}")
        if not isinstance(act, nn.ReLU):
            raise ValueError(f"{name}.{i + 3}: the HIP SAC head computes ReLU only, got {type(act).__name__}")
        lin.append((fc.weight, fc.bias))
        ln.append((norm.weight, norm.bias))
        ps.append(_dropout_of(dr.p))
        ts.append(bool(dr.training))
    return tuple(lin) + ((mods[-1].weight, mods[-1].bias),), tuple(ln), ps, ts


def _ens_desc(arch, n, actor=None, critic=None):
    """m3l_sac_ens_desc of n critics over the tensors of `actor` (actor_flat order) and / or `critic` (critic_flat order); the caller keeps them alive."""
    F, A, pi, qf = arch
    d = L.SacEnsDesc()
    d.features, d.actions, d.n_pi, d.n_qf, d.n_critics = F, A, len(pi), len(qf), n
    for l, w in enumerate(pi):
        d.pi_width[l] = w
    for l, w in enumerate(qf):
        d.qf_width[l] = w
    if actor is not None:
        it = iter(actor)
        for l in range(len(pi)):
            d.pi_weight[l], d.pi_bias[l] = next(it).data_ptr(), next(it).data_ptr()
        d.mu_weight, d.mu_bias = next(it).data_ptr(), next(it).data_ptr()
        d.log_std_weight, d.log_std_bias = next(it).data_ptr(), next(it).data_ptr()
    if critic is not None:
        it = iter(critic)
        for c in range(n):
            for l in range(len(qf)):
                d.qf_weight[c][l], d.qf_bias[c][l] = next(it).data_ptr(), next(it).data_ptr()
            d.q_weight[c], d.q_bias[c] = next(it).data_ptr(), next(it).data_ptr()
    return d


class SACEnsCriticFn(torch.autograd.Function):
    """(features (B, F), actions (B, A), arch, n, store, param_grads, *critic parameters in critic_flat order) -> q (n, B).  One launch.  The
    backward returns d actions (1 launch) and, with param_grads, every critic gradient (ceil(n * layers / 8) more); the features never take a
    gradient."""

    @staticmethod
    def forward(ctx, x, actions, arch, n, store, param_grads, *params):
        B = x.shape[0]
        flat = [_dev(t) for t in params]
        lib = L.lib()
        d = _ens_desc(arch, n, critic=flat)
        q = torch.empty(n, B, dtype=torch.float32, device=x.device)
        ws = _ws(lib.m3l_sac_ens_ws_bytes(C.byref(d), B), x.device) if store else None
        L.check(lib.m3l_sac_ens_critic_fwd(C.byref(d), B, L.ptr(x), L.ptr(actions), L.ptr(ws), L.ptr(q), _stream()), "m3l_sac_ens_critic_fwd")
        ctx.saved = (arch, n, flat, ws, B, bool(param_grads))
        return q

    @staticmethod
    def backward(ctx, dq):
        arch, n, flat, ws, B, param_grads = ctx.saved
        if ws is None:
            raise H.no_workspace("SACEnsCriticFn")
        dq = _dev(dq).reshape(n, B)
        dactions = torch.empty(B, arch[1], dtype=torch.float32, device=dq.device) if ctx.needs_input_grad[1] else None
        grads = [torch.empty_like(t) for t in flat] if param_grads else None
        d = _ens_desc(arch, n, critic=flat)
        gd = C.byref(_ens_desc(arch, n, critic=grads)) if param_grads else None
        L.check(L.lib().m3l_sac_ens_critic_bwd(C.byref(d), B, L.ptr(dq), L.ptr(ws), L.ptr(dactions), gd, _stream()), "m3l_sac_ens_critic_bwd")
        return (None, dactions, None, None, None, None) + (tuple(grads) if param_grads else (None,) * len(flat))


def _droq_desc(arch, n, p, seed, actor=None, critic=None, ln=None):
    """m3l_sac_droq_desc: `_ens_desc` of the same arguments, the LayerNorm tensors `ln` (ln_flat order), the dropout rate and the call's seed."""
    d = L.SacDroqDesc()
    d.ens = _ens_desc(arch, n, actor, critic)
    if ln is not None:
        it = iter(ln)
        for c in range(n):
            for l in range(len(arch[3])):
                d.ln_weight[c][l], d.ln_bias[c][l] = next(it).data_ptr(), next(it).data_ptr()
    d.dropout_p, d.seed = p, seed
    return d


class SACDroqCriticFn(torch.autograd.Function):
    """`SACEnsCriticFn` for DroQ critics: (features, actions, arch, n, store, param_grads, p, seed, *critic parameters in critic_flat order, then
    the LayerNorm tensors in ln_flat order) -> q (n, B).  One launch.  The masks are not stored: the backward regenerates them from the seed
    kept here.  Backward: d actions (1 launch) and, with param_grads, every Linear gradient (ceil(n * layers / 8) launches) and every d gamma /
    d beta (1 more)."""

    @staticmethod
    def forward(ctx, x, actions, arch, n, store, param_grads, p, seed, *params):
        B = x.shape[0]
        n_lin = 2 * n * (len(arch[3]) + 1)
        flat = [_dev(t) for t in params]
        lib = L.lib()
        d = _droq_desc(arch, n, p, seed, critic=flat[:n_lin], ln=flat[n_lin:])
        q = torch.empty(n, B, dtype=torch.float32, device=x.device)
        ws = _ws(lib.m3l_sac_droq_ws_bytes(C.byref(d), B), x.device) if store else None
        L.check(lib.m3l_sac_droq_critic_fwd(C.byref(d), B, L.ptr(x), L.ptr(actions), L.ptr(ws), L.ptr(q), _stream()), "m3l_sac_droq_critic_fwd")
        ctx.saved = (arch, n, flat, n_lin, ws, B, bool(param_grads), p, seed)
        return q

    @staticmethod
    def backward(ctx, dq):
        arch, n, flat, n_lin, ws, B, param_grads, p, seed = ctx.saved
        if ws is None:
            raise H.no_workspace("SACDroqCriticFn")
        dq = _dev(dq).reshape(n, B)
        dactions = torch.empty(B, arch[1], dtype=torch.float32, device=dq.device) if ctx.needs_input_grad[1] else None
        grads = [torch.empty_like(t) for t in flat] if param_grads else None
        d = _droq_desc(arch, n, p, seed, critic=flat[:n_lin], ln=flat[n_lin:])
        gd = C.byref(_droq_desc(arch, n, 0.0, 0, critic=grads[:n_lin], ln=grads[n_lin:])) if param_grads else None
        L.check(L.lib().m3l_sac_droq_critic_bwd(C.byref(d), B, L.ptr(dq), L.ptr(ws), L.ptr(dactions), gd, _stream()), "m3l_sac_droq_critic_bwd")
        return (None, dactions) + (None,) * 6 + (tuple(grads) if param_grads else (None,) * len(flat))


class SACEnsCriticLossFn(torch.autograd.Function):
    """(q (n, B), target_q (B,), weights (B,) or None, want_td) -> (0.5 * sum_c mean(weights * (q_c - target_q)^2) 0-d, td_abs (B,) = the mean over
    the critics of |q_c - target_q|, no gradient; an empty tensor without want_td).  One launch each way; the gradient goes to q."""

    @staticmethod
    def forward(ctx, q, target_q, weights, want_td):
        n, B = q.shape
        loss = torch.empty((), dtype=torch.float32, device=q.device)
        coef = torch.empty(n, B, dtype=torch.float32, device=q.device)
        td_abs = torch.empty(B if want_td else 0, dtype=torch.float32, device=q.device)
        L.check(L.lib().m3l_sac_ens_critic_loss_fwd(L.ptr(q), L.ptr(target_q), L.ptr(weights), n, B, L.ptr(loss), L.ptr(coef),
                                                    L.ptr(td_abs) if want_td else None, _stream()), "m3l_sac_ens_critic_loss_fwd")
        ctx.saved = coef
        ctx.mark_non_differentiable(td_abs)
        return loss, td_abs

    @staticmethod
    def backward(ctx, dloss, _dtd):
        coef = ctx.saved
        return H.scale_coef(dloss, coef), None, None, None


class SACEnsActorLossFn(torch.autograd.Function):
    """(log_prob (B,), q (n, B), reduce 0 = min / 1 = mean, ent_coef float or None, log_ent_coef tensor or None) -> the actor loss, 0-d.  One
    launch each way; the gradient goes to log_prob and q, the entropy coefficient is a constant."""

    @staticmethod
    def forward(ctx, logp, q, reduce, ent_coef, log_ent_coef):
        n, B = q.shape
        loss = torch.empty((), dtype=torch.float32, device=q.device)
        coef = torch.empty(1 + n, B, dtype=torch.float32, device=q.device)
        L.check(L.lib().m3l_sac_ens_actor_loss_fwd(L.ptr(logp), L.ptr(q), n, B, reduce, 0.0 if ent_coef is None else float(ent_coef), L.ptr(log_ent_coef),
                                                   L.ptr(loss), L.ptr(coef), _stream()), "m3l_sac_ens_actor_loss_fwd")
        ctx.saved = coef
        return loss

    @staticmethod
    def backward(ctx, dloss):
        coef = ctx.saved
        out = H.scale_coef(dloss, coef)
        return out[0], out[1:], None, None, None


def _q_of(q, what="q"):
    """q (N, B) float32 on the device, 1 <= N <= MAX_CRITICS -> (q contiguous, N, B)"""
    _require_cuda(q, what)
    if q.dim() != 2 or not 1 <= q.shape[0] <= MAX_CRITICS or q.shape[1] < 1 or q.dtype != torch.float32:
        raise ValueError(f"{what}: (N, B) float32 with 1 <= N <= {MAX_CRITICS} expected, got {tuple(q.shape)} {q.dtype}")
    return q.contiguous(), q.shape[0], q.shape[1]


def _reduce_of(q_reduce):
    if q_reduce not in Q_REDUCE:
        raise ValueError(f"q_reduce={q_reduce!r}: 'min' (SB3's n_critics semantics) or 'mean' (REDQ's actor loss) expected")
    return Q_REDUCE[q_reduce]


def _subset_of(subset, n):
    """The subset argument's form, checked without a device: None, or a contiguous int32 tensor of shape (M,), 1 <= M <= n."""
    if subset is None:
        return
    if not isinstance(subset, torch.Tensor) or subset.dtype != torch.int32 or subset.dim() != 1 or not subset.is_contiguous() or \
            not 1 <= subset.shape[0] <= n:
        form = f"{tuple(subset.shape)} {subset.dtype}" if isinstance(subset, torch.Tensor) else type(subset).__name__
        raise ValueError(f"subset: None, or a contiguous int32 tensor of shape (M,) with 1 <= M <= {n} critic indices expected (sample_subset "
                         f"makes one), got {form}")


def _ln_of(params, arch, target):
    """The LayerNorm tensors of DroQ critics (ln_flat order) with their form checked against the hidden widths; [] without LayerNorm."""
    if not params.layer_norm:
        return []
    for stem, nets in (("qf_ln", params.qf_ln), ("qf_target_ln", params.qf_target_ln)):
        if len(nets) != params.n_critics:
            raise ValueError(f"{stem}: {len(nets)} entries for {params.n_critics} critics")
        for i, net in enumerate(nets):
            if len(net) != len(arch[3]) or any(tuple(t.shape) != (w,) for (g, b), w in zip(net, arch[3]) for t in (g, b)):
                raise ValueError(f"{stem}{i}: one LayerNorm (weight, bias) of each hidden width {arch[3]} expected, got "
                                 f"{[tuple(g.shape) for g, _ in net]}")
    flat = params.ln_flat(target)
    H.check_float32(flat, "SAC")
    H.require_params(flat, "SAC head parameter")
    return flat


def _call_seed(params, target, dropout_seed):
    """(rate, seed) of a call on DroQ critics: the sub-module's rate and the injected seed, or a fresh draw; (0.0, 0) when nothing drops."""
    p = params.active_dropout(target)
    if p <= 0.0:
        return 0.0, 0
    return p, draw_seed() if dropout_seed is None else _seed_of(dropout_seed)


def q_values(params: SACEnsembleParams, features, actions, target=False, param_grads=True, dropout_seed=None):
    """q (N, B) of all critics (the target critics with target=True) at cat([features, actions]); differentiable in the actions and, unless
    param_grads=False, the critics' parameters; the features enter detached.  Under `no_grad`, or when nothing requires a gradient, no workspace
    is sized or stored.  dropout_seed: the seed of the masks of DroQ critics that drop (None: one draw from torch's CPU generator)."""
    flat = params.critic_flat(target)
    H.require_params(flat, "SAC head parameter")
    x = H.features_of(features, on_tape=False)
    arch = S._arch(x.shape[1], params)
    ln = _ln_of(params, arch, target)
    a = H.actions_of(actions, x.shape[0], arch[1])
    want = param_grads and any(t.requires_grad for t in flat + ln)
    store = torch.is_grad_enabled() and (a.requires_grad or want)
    if not params.layer_norm:
        return SACEnsCriticFn.apply(x, a, arch, params.n_critics, store, want, *flat)
    p, seed = _call_seed(params, target, dropout_seed)
    return SACDroqCriticFn.apply(x, a, arch, params.n_critics, store, want, p, seed, *flat, *ln)


@torch.no_grad()
def td_target(params: SACEnsembleParams, next_features, rewards, dones, gamma, ent_coef=None, log_ent_coef=None, noise=None, subset=None,
              dropout_seed=None):
    """target_q (B,) = r + (1 - done) * gamma * (min over the subset of q_target_c(x', a') - ent_coef * logp') with (a', logp') = actor(x').  One
    launch, no tape; only the critics of `subset` are evaluated.  gamma: a number, or one discount per row as `m3l_amd.sac.td_target` takes it.
    subset: None (all N critics) or int32 (M,) on the parameters' device, as `sample_subset` draws it; duplicates are harmless; an index outside
    [0, N) cannot be seen from the host without a read-back and makes every row NaN.  dropout_seed: as in `q_values`; DroQ target critics drop
    while `critic_target` is in train mode, each under its own index's masks whatever its place in the subset."""
    _subset_of(subset, params.n_critics)
    af, cf = params.actor_flat(), params.critic_flat(True)
    H.require_params(af + cf, "SAC head parameter")
    x = H.features_of(next_features, on_tape=False)
    arch = S._arch(x.shape[1], params)
    ln = _ln_of(params, arch, True)
    B = x.shape[0]
    if subset is not None:
        _require_cuda(subset, "subset")
        if subset.device != x.device:
            raise ValueError(f"subset lives on {subset.device}, the features on {x.device}")
    noise = H.noise_of(noise, B, arch[1], x.device)
    ent, log_ent = S._ent_args(ent_coef, log_ent_coef)
    r, dn = _vec(rewards, "rewards", B), _vec(dones, "dones", B)
    per_row, gamma = S._gamma_of(gamma, B)
    af, cf = [_dev(t) for t in af], [_dev(t) for t in cf]
    out = torch.empty(B, dtype=torch.float32, device=x.device)
    if params.layer_norm:
        ln = [_dev(t) for t in ln]
        p, seed = _call_seed(params, True, dropout_seed)
        d, entry = _droq_desc(arch, params.n_critics, p, seed, actor=af, critic=cf, ln=ln), "m3l_sac_droq_td_target"
    else:
        d, entry = _ens_desc(arch, params.n_critics, actor=af, critic=cf), "m3l_sac_ens_td_target"
    L.check(getattr(L.lib(), entry)(C.byref(d), B, L.ptr(x), L.ptr(noise), L.ptr(r), L.ptr(dn), L.ptr(gamma) if per_row else None,
                                    0.0 if per_row else gamma, 0.0 if ent is None else ent, L.ptr(log_ent), L.ptr(subset),
                                    0 if subset is None else subset.shape[0], L.ptr(out), _stream()), entry)
    return out


def critic_loss_from(q, target_q, weights=None, return_td_errors=False):
    """0.5 * sum_c mean(weights * (q_c - target_q)^2) from q (N, B) of `q_values`; weights (B,) or (B, 1) float32 or None (ones).
    return_td_errors: (loss, td) with td (B,) the mean over the critics of |q_c - target_q|, detached: what `update_priorities` takes."""
    q, _, B = _q_of(q)
    weights = H.weights_of(weights, B)
    loss, td = SACEnsCriticLossFn.apply(q, _vec(target_q, "target_q", B), weights, bool(return_td_errors))
    return (loss, td) if return_td_errors else loss


def actor_loss_from(log_prob, q, ent_coef=None, log_ent_coef=None, q_reduce="min"):
    """mean(ent_coef * log_prob - min_c q_c), or with q_reduce="mean" mean(ent_coef * log_prob - mean_c q_c), from the outputs of
    `m3l_amd.sac.action_log_prob` and `q_values`."""
    reduce = _reduce_of(q_reduce)
    _require_cuda(log_prob, "log_prob")
    q, _, B = _q_of(q)
    if log_prob.numel() != B or log_prob.dtype != torch.float32:
        raise ValueError(f"log_prob: ({B},) float32 expected beside q {tuple(q.shape)}, got {tuple(log_prob.shape)} {log_prob.dtype}")
    ent, log_ent = S._ent_args(ent_coef, log_ent_coef)
    return SACEnsActorLossFn.apply(log_prob.contiguous().reshape(B), q, reduce, ent, log_ent)


def _droq_mlp(k, widths, p):
    """[Linear, Dropout(p), LayerNorm, ReLU] per hidden width, then Linear(., 1): Linears at 4 l, LayerNorms at 4 l + 2, the output at 4 n."""
    mods = []
    for w in widths:
        mods += [nn.Linear(k, w), nn.Dropout(p), nn.LayerNorm(w, eps=1e-5), nn.ReLU()]
        k = w
    return nn.Sequential(*mods, nn.Linear(k, 1))


class _Critic(nn.Module):
    def __init__(self, features_dim, qf, action_dim, n_critics, layer_norm=False, dropout=0.0):
        super().__init__()
        self.n_critics, self.share_features_extractor = n_critics, True
        for i in range(n_critics):
            k = features_dim + action_dim
            setattr(self, f"qf{i}", _droq_mlp(k, qf, dropout) if layer_norm else H.mlp(k, qf, nn.ReLU, out=1))


class SACEnsembleHead(nn.Module):
    """`SACHead` with `n_critics` critics (1 to 10, default 10): the parameters of SB3's `SACPolicy(n_critics=N)` behind the features extractor
    under SB3's names (`critic.qf{0..N-1}`, `critic_target.qf{0..N-1}`), so an SB3 state dict with that `n_critics` loads with strict=True, and
    the head's part of a gradient step on the HIP kernels.  The REDQ loop is G critic updates per environment step, each `td_target(...,
    subset=head.sample_subset(2))` and `critic_loss`, then one `actor_loss(..., q_reduce="mean")`.  Parity with SB3 is unpinned.

    critic_layer_norm=True makes every critic and target critic `[Linear, Dropout(critic_dropout), LayerNorm, ReLU] x n_qf + Linear(., 1)`
    (keys `qf{c}.{4l}` Linear, `qf{c}.{4l+2}` LayerNorm, `qf{c}.{4 n_qf}` output; the Dropout module is there at p = 0 too): DroQ (Hiraoka et al.
    2022) with `n_critics=2, critic_dropout=0.01`, plain LayerNorm critics with p = 0; critic_dropout > 0 needs critic_layer_norm=True.  Dropout
    follows nn.Dropout's rule per sub-module: the critics drop while `head.critic` is in train mode, the target critics inside `td_target`
    while `head.critic_target` is (the constructor leaves both so: the DroQ paper's rule; `head.critic_target.eval()` is SB3's).  Every call
    that drops draws one 63-bit seed from torch's default CPU generator, kept in `last_dropout_seeds`; `dropout_seed=` injects one.  With both
    arguments at their defaults the head is the one described above, module for module and launch for launch."""

    def __init__(self, features_dim, action_dim, net_arch=None, n_critics=10, activation_fn=nn.ReLU, use_sde=False, share_features_extractor=True,
                 critic_layer_norm=False, critic_dropout=0.0):
        super().__init__()
        if activation_fn is not nn.ReLU:
            raise ValueError(f"activation_fn={getattr(activation_fn, '__name__', activation_fn)}: the HIP SAC head computes ReLU only")
        self.use_sde, self.share_features_extractor = bool(use_sde), bool(share_features_extractor)
        S._reject_flags(self)
        self.n_critics = _n_critics_of(n_critics)
        if not isinstance(critic_layer_norm, bool):
            raise ValueError(f"critic_layer_norm={critic_layer_norm!r}: True or False expected")
        self.critic_layer_norm, self.critic_dropout = critic_layer_norm, _dropout_of(critic_dropout)
        if self.critic_dropout > 0.0 and not critic_layer_norm:
            raise ValueError(f"critic_dropout={critic_dropout!r} without critic_layer_norm=True: the HIP critics drop in front of a LayerNorm only "
                             "(DroQ's Linear -> Dropout -> LayerNorm -> ReLU)")
        self.last_dropout_seeds = {"q_values": None, "td_target": None}
        self.features_dim, self.action_dim, pi, qf = H.head_dims(features_dim, action_dim, net_arch, [256, 256], "qf", "SAC", "net")
        self.actor = S._Actor(self.features_dim, pi, self.action_dim)
        self.critic = _Critic(self.features_dim, qf, self.action_dim, self.n_critics, critic_layer_norm, self.critic_dropout)
        self.critic_target = _Critic(self.features_dim, qf, self.action_dim, self.n_critics, critic_layer_norm, self.critic_dropout)
        self.critic_target.load_state_dict(self.critic.state_dict())
        self.critic_target.requires_grad_(False)

    def _seed(self, what, params, target, dropout_seed):
        """The seed of a call that drops (injected, or one draw from torch's CPU generator), kept in last_dropout_seeds; None when nothing drops."""
        if not params.layer_norm or params.active_dropout(target) <= 0.0:
            return None
        self.last_dropout_seeds[what] = draw_seed() if dropout_seed is None else _seed_of(dropout_seed)
        return self.last_dropout_seeds[what]

    def params(self) -> SACEnsembleParams:
        return SACEnsembleParams.from_policy(self)

    @torch.no_grad()
    def forward(self, features, deterministic=False, noise=None):
        """actions (B, A), no gradient: SB3's `_predict` after `extract_features`."""
        return S.action_log_prob(self.params(), features, noise, deterministic)[0]

    def action_log_prob(self, features, noise=None):
        return S.action_log_prob(self.params(), features, noise)

    def q_values(self, features, actions, target=False, dropout_seed=None):
        p = self.params()
        return q_values(p, features, actions, target, dropout_seed=self._seed("q_values", p, target, dropout_seed))

    def sample_subset(self, m):
        """M distinct critic indices, int32 (M,) on the parameters' device, drawn under torch's generator; nothing is read back."""
        if isinstance(m, bool) or not isinstance(m, numbers.Integral) or not 1 <= m <= self.n_critics:
            raise ValueError(f"sample_subset({m!r}): an integer from 1 to n_critics={self.n_critics} expected")
        return torch.randperm(self.n_critics, device=self.actor.mu.weight.device)[:int(m)].to(torch.int32)

    def td_target(self, next_features, rewards, dones, gamma, ent_coef=None, log_ent_coef=None, noise=None, subset=None, dropout_seed=None):
        p = self.params()
        return td_target(p, next_features, rewards, dones, gamma, ent_coef, log_ent_coef, noise, subset,
                         dropout_seed=self._seed("td_target", p, True, dropout_seed))

    def critic_loss(self, features, actions, target_q, weights=None, return_td_errors=False, dropout_seed=None):
        """0.5 * sum_c mean(weights * (q_c(features, actions) - target_q)^2), and the td errors for `update_priorities` when asked for."""
        with torch.no_grad():
            a = actions.detach()
        p = self.params()
        q = q_values(p, features, a, dropout_seed=self._seed("q_values", p, False, dropout_seed))
        return critic_loss_from(q, target_q, weights, return_td_errors)

    def actor_loss(self, features, ent_coef=None, log_ent_coef=None, noise=None, q_reduce="min", dropout_seed=None):
        """(loss, log_prob.detach()): mean(ent_coef * log_prob - reduce_c q_c(features, a_pi)) with reduce "min" or "mean".  The critics give
        their gradient in the actions only: their parameters receive nothing from this loss."""
        _reduce_of(q_reduce)
        p = self.params()
        a_pi, logp = S.action_log_prob(p, features, noise)
        q = q_values(p, features, a_pi, param_grads=False, dropout_seed=self._seed("q_values", p, False, dropout_seed))
        return actor_loss_from(logp, q, ent_coef, log_ent_coef, q_reduce), logp.detach()

    def ent_coef_loss(self, log_ent_coef, log_prob, target_entropy):
        return S.ent_coef_loss(log_ent_coef, log_prob, target_entropy)

    @torch.no_grad()
    def polyak_update(self, tau):
        """critic_target = (1 - tau) * critic_target + tau * critic over every tensor of all N critics, in one multi-tensor launch."""
        update_moving_average(self.critic_target, self.critic, 1.0 - float(tau))
