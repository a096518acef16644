"""The SAC head with truncated quantile critics (TQC, Kuznetsov et al. 2020; `sb3_contrib.TQC`) on the HIP kernels of m3l_amd/csrc/sac.hip
("SAC TQC critics" of include/m3l_amd.h): N critics whose last Linear has `n_quantiles` outputs, a target made of the pooled, sorted and
truncated quantiles of the target critics, and the pairwise quantile-Huber loss.

  rule  : z_c = critic_c(cat([x, a])) (B, nq) per critic, the ensemble's critic with a wider head;  quantiles (N, B, nq);
          target (B, K) = r + (1 - done) * gamma * (the K = N * (nq - d) smallest of the N * nq target quantiles at (x', a') - ent_coef * logp');
          critic_loss = mean over (b, c, j, k) of weights_b * |tau_j - [delta < 0]| * huber(delta), delta = target[b, k] - z[c, b, j],
          tau_j = (j + 0.5) / nq, td = the row's mean |delta|;  actor_loss = mean(ent_coef * logp - mean_{c, j} z[c, b, j]).
  nodes : the actor's are `m3l_amd.sac`'s (`SACActorFn`, the entropy-coefficient loss); `TQCCriticFn` (1 launch forward; backward 1 chain launch
          + ceil(N * (layers per critic) / 8) weight-gradient launches), `TQCCriticLossFn` (2 + 1) and `TQCActorLossFn` (1 + 1).  `td_target` is
          one launch without a tape: the sort runs inside it.  Nothing is read back to the host.

sb3-contrib is not part of the reference tree: PARITY UNPINNED; tests/tqc_cases.py restates the rule in float64 as sb3-contrib writes it.
Not computed: `subset=` (REDQ-style subsets of quantile critics), LayerNorm / dropout critics under TQC, `sum_over_quantiles=True`, and the
actor-side changes of later TQC variants.  `SACHead` and `SACEnsembleHead` are unchanged.  Everything is float32; there is no eager fallback."""
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
from .sac_ensemble import _ens_desc, _n_critics_of

MAX_QUANTILES, MAX_POOL = L.TQC_MAX_QUANTILES, L.TQC_MAX_POOL


def _counts_of(n_critics, n_quantiles, drop):
    """(N, nq, d) as ints inside the kernels' limits."""
    n = _n_critics_of(n_critics)
    if isinstance(n_quantiles, bool) or not isinstance(n_quantiles, numbers.Integral) or not 1 <= n_quantiles <= MAX_QUANTILES:
        raise ValueError(f"n_quantiles={n_quantiles!r}: an integer from 1 to {MAX_QUANTILES} expected (the width of the HIP head tile)")
    if isinstance(drop, bool) or not isinstance(drop, numbers.Integral) or not 0 <= drop < n_quantiles:
        raise ValueError(f"top_quantiles_to_drop_per_net={drop!r}: an integer with 0 <= d < n_quantiles={n_quantiles} expected")
    if n * n_quantiles > MAX_POOL:
        raise ValueError(f"n_critics * n_quantiles = {n} * {n_quantiles} = {n * n_quantiles} pooled target quantiles per row: the HIP target kernel "
                         f"sorts at most {MAX_POOL} in LDS")
    return n, int(n_quantiles), int(drop)


class _TQCFields(NamedTuple):
    pi: Tuple[WB, ...]
    mu: WB
    log_std: WB
    qf: Tuple[Tuple[WB, ...], ...]
    qf_target: Tuple[Tuple[WB, ...], ...]


class TQCParams(_TQCFields):
    """The parameter tensors of a TQC head, torch.nn.Linear layouts: `SACEnsembleParams`' five fields, the last Linear of every critic being
    Linear(., n_quantiles); `n_quantiles` and `top_quantiles_to_drop_per_net` ride along as attributes."""

    def __new__(cls, pi, mu, log_std, qf, qf_target, n_quantiles, top_quantiles_to_drop_per_net):
        self = super().__new__(cls, pi, mu, log_std, qf, qf_target)
        self.n_quantiles, self.top_quantiles_to_drop_per_net = n_quantiles, top_quantiles_to_drop_per_net
        return self

    @property
    def n_critics(self):
        return len(self.qf)

    @property
    def n_target_quantiles(self):
        """K: the target quantiles kept per row."""
        return self.n_critics * (self.n_quantiles - self.top_quantiles_to_drop_per_net)

    def actor_flat(self):
        return [t for wb in self.pi for t in wb] + list(self.mu) + list(self.log_std)

    def critic_flat(self, target=False):
        return [t for net in (self.qf_target if target else self.qf) for wb in net for t in wb]

    @staticmethod
    def from_policy(policy, top_quantiles_to_drop_per_net=None) -> "TQCParams":
        """From a module with sb3-contrib's attribute names (`actor.latent_pi / mu / log_std`, `critic.qf0 .. qf{N-1}` and `critic.n_quantiles`,
        the same for `critic_target`): a `TQCHead`, or an sb3-contrib `TQCPolicy`, whose configuration is checked against what the kernels
        compute.  top_quantiles_to_drop_per_net: sb3-contrib keeps it on the algorithm, not the policy; None reads the policy's attribute."""
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
        if counts[1] != counts[0]:
            raise ValueError(f"{counts[0]} critics and {counts[1]} target critics: the two must agree")
        if top_quantiles_to_drop_per_net is None:
            if not hasattr(policy, "top_quantiles_to_drop_per_net"):
                raise ValueError("top_quantiles_to_drop_per_net: the policy does not carry it (sb3-contrib keeps it on the algorithm): pass it")
            top_quantiles_to_drop_per_net = policy.top_quantiles_to_drop_per_net
        first = list(getattr(policy.critic, "qf0", []))
        nq = getattr(policy.critic, "n_quantiles", first[-1].out_features if first and isinstance(first[-1], nn.Linear) else None)
        n, nq, drop = _counts_of(counts[0], nq, top_quantiles_to_drop_per_net)
        for name, c in (("critic", policy.critic), ("critic_target", policy.critic_target)):
            if getattr(c, "n_quantiles", nq) != nq:
                raise ValueError(f"{name}: n_quantiles={c.n_quantiles}, the critics have {nq}")
        pi, mu, log_std = S._read_policy(_ActorOnly(policy), 0)[:3]
        qf = tuple(_z_net(getattr(policy.critic, f"qf{i}"), f"critic.qf{i}", nq) for i in range(n))
        qt = tuple(_z_net(getattr(policy.critic_target, f"qf{i}"), f"critic_target.qf{i}", nq) for i in range(n))
        return TQCParams(pi, mu, log_std, qf, qt, nq, drop)


class _ActorOnly:
    """The actor's side of a policy for `S._read_policy` with no critics."""

    def __init__(self, policy):
        self.actor, self.critic, self.critic_target = policy.actor, policy.critic, policy.critic_target


def _z_net(seq, name, nq):
    mods = list(seq)
    if not mods or not isinstance(mods[-1], nn.Linear) or mods[-1].bias is None or mods[-1].out_features != nq:
        raise ValueError(f"{name}: a net ending in nn.Linear(., {nq}) with a bias expected (LayerNorm / dropout critics are not computed under TQC)")
    return H.linear_pairs(mods[:-1], name, nn.ReLU, "SAC") + ((mods[-1].weight, mods[-1].bias),)


def _arch(F, params: TQCParams):
    """(F, A, pi widths, qf widths) with every shape checked, as `m3l_amd.sac._arch` does it for heads of one output."""
    F = int(F)
    A = int(params.mu[0].shape[0])
    n, nq, _ = _counts_of(params.n_critics, params.n_quantiles, params.top_quantiles_to_drop_per_net)
    H.check_float32(params.actor_flat() + params.critic_flat() + params.critic_flat(True), "SAC")
    k, pi = H.layer_widths(F, params.pi, "pi", "SAC", "net")
    H.check_head_linear("mu", params.mu, A, k)
    H.check_head_linear("log_std", params.log_std, A, k)
    qf = None
    for stem, nets in (("qf", params.qf), ("qf_target", params.qf_target)):
        if len(nets) != n:
            raise ValueError(f"{stem}: {len(nets)} critics: the HIP TQC head computes 1 to {MAX_CRITICS} critics and as many targets")
        for i, net in enumerate(nets):
            name = f"{stem}{i}"
            k, ws = H.layer_widths(F + A, net[:-1], name, "SAC", "net")
            H.check_head_linear(f"{name} layer {len(net) - 1}", net[-1], nq, k)
            if qf is not None and ws != qf:
                raise ValueError(f"{name}: hidden widths {ws}, the other critics have {qf}: the {n} critics and their targets must be alike")
            qf = ws
    H.check_limits((F,) + pi + qf, A)
    return F, A, pi, qf


def _desc(arch, params, actor=None, critic=None):
    """m3l_tqc_desc: `_ens_desc` of the same arguments, then the two quantile counts."""
    d = L.TqcDesc()
    d.ens = _ens_desc(arch, params.n_critics, actor, critic)
    d.n_quantiles, d.top_quantiles_to_drop = params.n_quantiles, params.top_quantiles_to_drop_per_net
    return d


class _Counts(NamedTuple):
    """What `_desc` reads of a TQCParams, for the autograd nodes (which keep no parameter tuple)."""
    n_critics: int
    n_quantiles: int
    top_quantiles_to_drop_per_net: int


class TQCCriticFn(torch.autograd.Function):
    """(features (B, F), actions (B, A), arch, counts, store, param_grads, *critic parameters in critic_flat order) -> z (N, B, nq).  One launch.
    The backward returns d actions (1 launch) and, with param_grads, every critic gradient (ceil(N * layers / 8) more); the features never
    take a gradient."""

    @staticmethod
    def forward(ctx, x, actions, arch, counts, store, param_grads, *params):
        B = x.shape[0]
        flat = [_dev(t) for t in params]
        lib = L.lib()
        d = _desc(arch, counts, critic=flat)
        z = torch.empty(counts.n_critics, B, counts.n_quantiles, dtype=torch.float32, device=x.device)
        ws = _ws(lib.m3l_tqc_ws_bytes(C.byref(d), B), x.device) if store else None
        L.check(lib.m3l_tqc_critic_fwd(C.byref(d), B, L.ptr(x), L.ptr(actions), L.ptr(ws), L.ptr(z), _stream()), "m3l_tqc_critic_fwd")
        ctx.saved = (arch, counts, flat, ws, B, bool(param_grads))
        return z

    @staticmethod
    def backward(ctx, dz):
        arch, counts, flat, ws, B, param_grads = ctx.saved
        if ws is None:
            raise H.no_workspace("TQCCriticFn")
        dz = _dev(dz).reshape(counts.n_critics, B, counts.n_quantiles)
        dactions = torch.empty(B, arch[1], dtype=torch.float32, device=dz.device) if ctx.needs_input_grad[1] else None
        grads = [torch.empty_like(t) for t in flat] if param_grads else None
        d = _desc(arch, counts, critic=flat)
        gd = C.byref(_desc(arch, counts, critic=grads)) if param_grads else None
        L.check(L.lib().m3l_tqc_critic_bwd(C.byref(d), B, L.ptr(dz), L.ptr(ws), L.ptr(dactions), gd, _stream()), "m3l_tqc_critic_bwd")
        return (None, dactions, None, None, None, None) + (tuple(grads) if param_grads else (None,) * len(flat))


class TQCCriticLossFn(torch.autograd.Function):
    """(z (N, B, nq), target (B, K), weights (B,) or None, want_td) -> (the quantile-Huber loss 0-d, td_abs (B,) = the row's mean |delta|, no
    gradient; an empty tensor without want_td).  Two launches forward (row tiles x critics, then the fixed-order finish), one backward; the
    gradient goes to z."""

    @staticmethod
    def forward(ctx, z, target, weights, want_td):
        n, B, nq = z.shape
        K = target.shape[1]
        lib = L.lib()
        loss = torch.empty((), dtype=torch.float32, device=z.device)
        coef = torch.empty(n, B, nq, dtype=torch.float32, device=z.device)
        td_abs = torch.empty(B if want_td else 0, dtype=torch.float32, device=z.device)
        scratch = _ws(lib.m3l_tqc_loss_ws_bytes(n, B), z.device)
        L.check(lib.m3l_tqc_critic_loss_fwd(L.ptr(z), L.ptr(target), L.ptr(weights), n, B, nq, K, L.ptr(scratch), L.ptr(loss), L.ptr(coef),
                                            L.ptr(td_abs) if want_td else None, _stream()), "m3l_tqc_critic_loss_fwd")
        ctx.saved = coef
        ctx.mark_non_differentiable(td_abs)
        return loss, td_abs

    @staticmethod
    def backward(ctx, dloss, _dtd):
        coef = ctx.saved
        return H.scale_coef(dloss, coef), None, None, None


class TQCActorLossFn(torch.autograd.Function):
    """(log_prob (B,), z (N, B, nq), ent_coef float or None, log_ent_coef tensor or None) -> mean(ent_coef * log_prob - mean_{c, j} z), 0-d.  One
    launch each way; the gradient goes to log_prob and z, the entropy coefficient is a constant."""

    @staticmethod
    def forward(ctx, logp, z, ent_coef, log_ent_coef):
        n, B, nq = z.shape
        loss = torch.empty((), dtype=torch.float32, device=z.device)
        coef = torch.empty(B + n * B * nq, dtype=torch.float32, device=z.device)
        L.check(L.lib().m3l_tqc_actor_loss_fwd(L.ptr(logp), L.ptr(z), n, B, nq, 0.0 if ent_coef is None else float(ent_coef), L.ptr(log_ent_coef),
                                               L.ptr(loss), L.ptr(coef), _stream()), "m3l_tqc_actor_loss_fwd")
        ctx.saved = (coef, tuple(z.shape))
        return loss

    @staticmethod
    def backward(ctx, dloss):
        coef, shape = ctx.saved
        out = H.scale_coef(dloss, coef)
        B = shape[1]
        return out[:B], out[B:].reshape(shape), None, None


def _z_of(z, what="quantiles"):
    """z (N, B, nq) float32 on the device inside the limits -> z contiguous"""
    _require_cuda(z, what)
    if z.dim() != 3 or not 1 <= z.shape[0] <= MAX_CRITICS or z.shape[1] < 1 or not 1 <= z.shape[2] <= MAX_QUANTILES or z.dtype != torch.float32:
        raise ValueError(f"{what}: (N, B, n_quantiles) float32 with 1 <= N <= {MAX_CRITICS} and 1 <= n_quantiles <= {MAX_QUANTILES} expected, got "
                         f"{tuple(z.shape)} {z.dtype}")
    return z.contiguous()


def action_log_prob(params: TQCParams, features, noise=None, deterministic=False):
    """`m3l_amd.sac.action_log_prob` (the same node, `SACActorFn`) on the actor of a TQC head."""
    flat = params.actor_flat()
    H.require_params(flat, "SAC head parameter")
    x = H.features_of(features, on_tape=True)
    arch = _arch(x.shape[1], params)
    noise = H.noise_of(noise, x.shape[0], arch[1], x.device, deterministic)
    store = torch.is_grad_enabled() and (x.requires_grad or any(t.requires_grad for t in flat))
    return S.SACActorFn.apply(x, noise, arch, store, *flat)


def quantiles(params: TQCParams, features, actions, target=False, param_grads=True):
    """z (N, B, nq) of all critics (the target critics with target=True) at cat([features, actions]), contiguous; differentiable in the actions
    and, unless param_grads=False, the critics' parameters; the features enter detached.  Under `no_grad`, or when nothing requires a gradient,
    no workspace is sized or stored."""
    flat = params.critic_flat(target)
    H.require_params(flat, "SAC head parameter")
    x = H.features_of(features, on_tape=False)
    arch = _arch(x.shape[1], params)
    a = H.actions_of(actions, x.shape[0], arch[1])
    want = param_grads and any(t.requires_grad for t in flat)
    store = torch.is_grad_enabled() and (a.requires_grad or want)
    counts = _Counts(params.n_critics, params.n_quantiles, params.top_quantiles_to_drop_per_net)
    return TQCCriticFn.apply(x, a, arch, counts, store, want, *flat)


@torch.no_grad()
def td_target(params: TQCParams, next_features, rewards, dones, gamma, ent_coef=None, log_ent_coef=None, noise=None):
    """target (B, K) = r + (1 - done) * gamma * (the K = N * (nq - d) smallest pooled target quantiles at (x', a'), ascending, - ent_coef * logp')
    with (a', logp') = actor(x').  One launch, no tape.  gamma: a number, or one discount per row as `m3l_amd.sac.td_target` takes it (the
    `discounts` of an `NStepReplayBatch`)."""
    af, cf = params.actor_flat(), params.critic_flat(True)
    H.require_params(af + cf, "SAC head parameter")
    x = H.features_of(next_features, on_tape=False)
    arch = _arch(x.shape[1], params)
    B = x.shape[0]
    noise = H.noise_of(noise, B, arch[1], x.device)
    ent, log_ent = S._ent_args(ent_coef, log_ent_coef)
    r, dn = _vec(rewards, "rewards", B), _vec(dones, "dones", B)
    per_row, gamma = S._gamma_of(gamma, B)
    af, cf = [_dev(t) for t in af], [_dev(t) for t in cf]
    out = torch.empty(B, params.n_target_quantiles, dtype=torch.float32, device=x.device)
    d = _desc(arch, params, actor=af, critic=cf)
    L.check(L.lib().m3l_tqc_td_target(C.byref(d), B, L.ptr(x), L.ptr(noise), L.ptr(r), L.ptr(dn), L.ptr(gamma) if per_row else None,
                                      0.0 if per_row else gamma, 0.0 if ent is None else ent, L.ptr(log_ent), L.ptr(out), _stream()), "m3l_tqc_td_target")
    return out


def _loss_args(B, target, weights, K=None):
    """target (B, K) and weights (B,) or None as the loss kernel reads them, every form checked; nothing is launched."""
    if isinstance(target, torch.Tensor) and K is not None and (target.dim() != 2 or target.shape[1] != K):
        raise ValueError(f"target: (B, K = {K}) expected (n_critics * (n_quantiles - top_quantiles_to_drop_per_net)), got {tuple(target.shape)}")
    _require_cuda(target, "target")
    if target.dim() != 2 or target.shape[0] != B or not 1 <= target.shape[1] <= MAX_POOL or target.dtype != torch.float32:
        raise ValueError(f"target: ({B}, K) float32 with 1 <= K <= {MAX_POOL} expected, got {tuple(target.shape)} {target.dtype}")
    weights = H.weights_of(weights, B)
    return _dev(target), weights


def critic_loss_from(z, target, weights=None, return_td_errors=False):
    """The quantile-Huber loss of z (N, B, nq) from `quantiles` against target (B, K) from `td_target`, averaged over every (b, c, j, k) pair;
    weights (B,) or (B, 1) float32 or None (ones).  return_td_errors: (loss, td) with td (B,) the row's mean |target - z|, detached: what
    `DeviceReplayBuffer.update_priorities` takes."""
    z = _z_of(z)
    target, weights = _loss_args(z.shape[1], target, weights)
    loss, td = TQCCriticLossFn.apply(z, target, weights, bool(return_td_errors))
    return (loss, td) if return_td_errors else loss


def actor_loss_from(log_prob, z, ent_coef=None, log_ent_coef=None):
    """mean(ent_coef * log_prob - mean_{c, j} z[c, b, j]) from the outputs of `m3l_amd.sac.action_log_prob` and `quantiles`."""
    _require_cuda(log_prob, "log_prob")
    z = _z_of(z)
    B = z.shape[1]
    if log_prob.numel() != B or log_prob.dtype != torch.float32:
        raise ValueError(f"log_prob: ({B},) float32 expected beside quantiles {tuple(z.shape)}, got {tuple(log_prob.shape)} {log_prob.dtype}")
    ent, log_ent = S._ent_args(ent_coef, log_ent_coef)
    return TQCActorLossFn.apply(log_prob.contiguous().reshape(B), z, ent, log_ent)


class _Critic(nn.Module):
    def __init__(self, features_dim, qf, action_dim, n_critics, n_quantiles):
        super().__init__()
        self.n_critics, self.n_quantiles, self.quantiles_total = n_critics, n_quantiles, n_critics * n_quantiles
        self.share_features_extractor = True
        for i in range(n_critics):
            setattr(self, f"qf{i}", H.mlp(features_dim + action_dim, qf, nn.ReLU, out=n_quantiles))


class TQCHead(nn.Module):
    """`SACEnsembleHead` with quantile critics: the parameters of sb3-contrib's `TQCPolicy` behind the features extractor under its names
    (`actor.*`, `critic.qf{0..N-1}`, `critic_target.qf{0..N-1}`, each `qf{i}` Linear + ReLU pairs and a last Linear(., n_quantiles)), so a state
    dict with those names is meant to load with strict=True, and the head's part of a TQC gradient step on the HIP kernels: `td_target` ->
    `critic_loss` (PER weights and td errors as on `SACHead`) -> `actor_loss` -> `polyak_update`.  The target critics are a frozen copy.
    Parity with sb3-contrib is unpinned.  Not computed: `subset=`, LayerNorm / dropout critics, `sum_over_quantiles=True`."""

    def __init__(self, features_dim, action_dim, net_arch=None, n_critics=2, n_quantiles=25, top_quantiles_to_drop_per_net=2, activation_fn=nn.ReLU,
                 use_sde=False, share_features_extractor=True):
        super().__init__()
        if activation_fn is not nn.ReLU:
            raise ValueError(f"activation_fn={getattr(activation_fn, '__name__', activation_fn)}: the HIP SAC head computes ReLU only")
        self.use_sde, self.share_features_extractor = bool(use_sde), bool(share_features_extractor)
        S._reject_flags(self)
        self.n_critics, self.n_quantiles, self.top_quantiles_to_drop_per_net = _counts_of(n_critics, n_quantiles, top_quantiles_to_drop_per_net)
        self.features_dim, self.action_dim, pi, qf = H.head_dims(features_dim, action_dim, net_arch, [256, 256], "qf", "SAC", "net")
        self.actor = S._Actor(self.features_dim, pi, self.action_dim)
        self.critic = _Critic(self.features_dim, qf, self.action_dim, self.n_critics, self.n_quantiles)
        self.critic_target = _Critic(self.features_dim, qf, self.action_dim, self.n_critics, self.n_quantiles)
        self.critic_target.load_state_dict(self.critic.state_dict())
        self.critic_target.requires_grad_(False)

    @property
    def n_target_quantiles(self):
        """K = n_critics * (n_quantiles - top_quantiles_to_drop_per_net): the width of `td_target`'s result."""
        return self.n_critics * (self.n_quantiles - self.top_quantiles_to_drop_per_net)

    def params(self) -> TQCParams:
        return TQCParams.from_policy(self)

    @torch.no_grad()
    def forward(self, features, deterministic=False, noise=None):
        """actions (B, A), no gradient: SB3's `_predict` after `extract_features`."""
        return action_log_prob(self.params(), features, noise, deterministic)[0]

    def action_log_prob(self, features, noise=None):
        return action_log_prob(self.params(), features, noise)

    def quantiles(self, features, actions, target=False):
        return quantiles(self.params(), features, actions, target)

    def td_target(self, next_features, rewards, dones, gamma, ent_coef=None, log_ent_coef=None, noise=None):
        return td_target(self.params(), next_features, rewards, dones, gamma, ent_coef, log_ent_coef, noise)

    def critic_loss(self, features, actions, target, weights=None, return_td_errors=False):
        """The quantile-Huber loss of the critics at (features, actions) against `target` (B, K), and the td errors for `update_priorities` when
        asked for."""
        p = self.params()
        B = features.shape[0] if isinstance(features, torch.Tensor) and features.dim() == 2 else -1
        target, weights = _loss_args(B, target, weights, p.n_target_quantiles)          # refused before anything is launched
        with torch.no_grad():
            a = actions.detach()
        loss, td = TQCCriticLossFn.apply(quantiles(p, features, a), target, weights, bool(return_td_errors))
        return (loss, td) if return_td_errors else loss

    def actor_loss(self, features, ent_coef=None, log_ent_coef=None, noise=None):
        """(loss, log_prob.detach()): mean(ent_coef * log_prob - mean_{c, j} z[c, b, j](features, a_pi)).  The critics give their gradient in the
        actions only: their parameters receive nothing from this loss."""
        p = self.params()
        a_pi, logp = action_log_prob(p, features, noise)
        z = quantiles(p, features, a_pi, param_grads=False)
        return actor_loss_from(logp, z, ent_coef, log_ent_coef), logp.detach()

    def ent_coef_loss(self, log_ent_coef, log_prob, target_entropy):
        return S.ent_coef_loss(log_ent_coef, log_prob, target_entropy)

    @torch.no_grad()
    def polyak_update(self, tau):
        """critic_target = (1 - tau) * critic_target + tau * critic over every tensor of all N critics, in one multi-tensor launch."""
        update_moving_average(self.critic_target, self.critic, 1.0 - float(tau))
