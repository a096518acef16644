"""The deterministic-actor head on the HIP kernels of m3l_amd/csrc/sac.hip ("TD3 head" of include/m3l_amd.h): what DDPG (Lillicrap et al. 2016),
TD3 (Fujimoto et al. 2018; SB3's `TD3Policy`) and DrQ-v2 (Yarats et al. 2022) put behind the features extractor.

  rule  : mu(x) = tanh(Linear_A(ReLU-MLP(x)));  smooth(a, n, sigma, c) = clamp(a + clamp(sigma * n, -c, c), -1, 1) (c None: no inner clamp);
          actions = smooth(mu(x), noise, noise_std, noise_clip), both clamps passing the gradient straight through;
          target_q = r + (1 - done) * gamma * min_c q_target_c(x', smooth(mu_target(x'), noise, target_policy_noise, target_noise_clip));
          critic_loss = sum_c mean(weights * (q_c - target_q)^2) (SB3's TD3 line: twice the SAC head's, bit for bit), td = mean_c |q_c - target_q|;
          actor_loss = -mean(reduce_c q_c(x, actions)): "first" (SB3's q1_forward: only critic 0 runs), "min" (DrQ-v2) or "mean".
  nodes : `TD3ActorFn` (1 launch forward, 2 backward), the ensemble's `SACEnsCriticFn` for the critics, one node per loss (1 + 1).  `td_target`
          is one launch without a tape.  DDPG is n_critics=1 with no noise; DrQ-v2 is `td_target(..., use_actor_target=False)`, `actor_loss(...,
          q_reduce="min", noise_std=sigma, noise_clip=c)` and the sigma schedule in the caller's loop, like `policy_delay`.

Neither SB3 nor a DrQ-v2 implementation is part of the reference tree: PARITY UNPINNED; tests/td3_cases.py restates the rule in float64.
Everything is float32; there is no eager fallback."""
import ctypes as C
import math
import numbers
from typing import NamedTuple, Tuple

import torch
from torch import nn

from . import _head as H
from . import _lib as L
from . import sac_ensemble as SE
from ._head import _dev, _vec
from .dino import update_moving_average
from .functional import _stream, _ws
from .sac import MAX_CRITICS, WB, _gamma_of, _q_net

Q_REDUCE = {"first": 0, "min": 0, "mean": 1}          # the kernel's reduce code; "first" hands it critic 0 alone


class TD3Params(NamedTuple):
    """The parameter tensors of a head, torch.nn.Linear layouts.  pi / pi_target: (weight, bias) per hidden layer of the actor (the target
    actor); mu / mu_target: the action Linear; qf / qf_target: per critic, (weight, bias) of every Linear, the last one being the Linear(., 1)."""
    pi: Tuple[WB, ...]
    mu: WB
    pi_target: Tuple[WB, ...]
    mu_target: WB
    qf: Tuple[Tuple[WB, ...], ...]
    qf_target: Tuple[Tuple[WB, ...], ...]

    @property
    def n_critics(self):
        return len(self.qf)

    def actor_flat(self, target=False):
        pi, mu = (self.pi_target, self.mu_target) if target else (self.pi, self.mu)
        return [t for wb in pi for t in wb] + list(mu)

    def critic_flat(self, target=False):
        return [t for net in (self.qf_target if target else self.qf) for wb in net for t in wb]

    @staticmethod
    def from_policy(policy) -> "TD3Params":
        """From a module with SB3's `TD3Policy` attribute names (`actor.mu`, `actor_target.mu`, `critic.qf0 ..`, `critic_target.qf0 ..`): a
        `TD3Head`, or an SB3 policy, whose configuration is checked against what the kernels compute."""
        H.require_shared_extractor(policy, "TD3")
        counts = []
        for name in ("critic", "critic_target"):
            c = getattr(policy, name)
            H.require_shared_extractor(c, "TD3", name)
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
        n = SE._n_critics_of(counts[0])
        pi, mu = _actor_net(policy.actor.mu, "actor.mu")
        pit, mut = _actor_net(policy.actor_target.mu, "actor_target.mu")
        qf = tuple(_q_net(getattr(policy.critic, f"qf{i}"), f"critic.qf{i}") for i in range(n))
        qt = tuple(_q_net(getattr(policy.critic_target, f"qf{i}"), f"critic_target.qf{i}") for i in range(n))
        return TD3Params(pi, mu, pit, mut, qf, qt)


def _actor_net(seq, name):
    """(hidden (weight, bias) pairs, the action Linear's (weight, bias)) of SB3's `Actor.mu`: Linear / ReLU pairs, then Linear(., A) and Tanh."""
    mods = list(seq)
    if len(mods) < 2 or not isinstance(mods[-1], nn.Tanh) or not isinstance(mods[-2], nn.Linear) or mods[-2].bias is None:
        raise ValueError(f"{name}: a net ending in nn.Linear(., action_dim) with a bias and nn.Tanh expected (SB3's squash_output=True)")
    return H.linear_pairs(mods[:-2], name, nn.ReLU, "TD3"), (mods[-2].weight, mods[-2].bias)


def _arch(F, params):
    """(F, A, pi widths, qf widths) with every shape checked; raises ValueError for a head outside the kernels' limits."""
    F = int(F)
    A = int(params.mu[0].shape[0])
    H.check_float32(params.actor_flat() + params.actor_flat(True) + params.critic_flat() + params.critic_flat(True), "TD3")
    pi = None
    for stem, hidden, mu in (("actor", params.pi, params.mu), ("actor_target", params.pi_target, params.mu_target)):
        k, ws = H.layer_widths(F, hidden, stem, "TD3", "net")
        H.check_head_linear(stem + " action layer", mu, A, k)
        if pi is not None and ws != pi:
            raise ValueError(f"actor_target: hidden widths {ws}, the actor has {pi}: the actor and its target must be alike")
        pi = ws
    n = len(params.qf)
    qf = None
    for stem, nets in (("qf", params.qf), ("qf_target", params.qf_target)):
        if not 1 <= len(nets) <= MAX_CRITICS or len(nets) != n:
            raise ValueError(f"{stem}: {len(nets)} critics: the HIP TD3 head computes 1 to {MAX_CRITICS} critics and as many targets")
        for i, net in enumerate(nets):
            name = f"{stem}{i}"
            k, ws = H.layer_widths(F + A, net[:-1], name, "TD3", "net")
            w, b = net[-1]
            if tuple(w.shape) != (1, k) or tuple(b.shape) != (1,):
                raise ValueError(f"{name} layer {len(net) - 1}: weight {tuple(w.shape)} / bias {tuple(b.shape)} do not follow an input of width {k}")
            if qf is not None and ws != qf:
                raise ValueError(f"{name}: hidden widths {ws}, the other critics have {qf}: the {n} critics and their targets must be alike")
            qf = ws
    H.check_limits((F,) + pi + qf, A)
    return F, A, pi, qf


def _desc(arch, n, actor=None, critic=None):
    """m3l_sac_ens_desc of a TD3 head: the actor's tensors (actor_flat order) in pi_* and mu_*, log_std_* NULL, and / or n critics (critic_flat
    order); the caller keeps the tensors alive."""
    d = SE._ens_desc(arch, n, critic=critic)
    if actor is not None:
        it = iter(actor)
        for l in range(len(arch[2])):
            d.pi_weight[l], d.pi_bias[l] = next(it).data_ptr(), next(it).data_ptr()
        d.mu_weight, d.mu_bias = next(it).data_ptr(), next(it).data_ptr()
    return d


def _sigma_of(sigma, what):
    if isinstance(sigma, bool) or not isinstance(sigma, numbers.Real) or not math.isfinite(sigma) or sigma < 0:
        raise ValueError(f"{what}={sigma!r}: a finite number >= 0 expected")
    return float(sigma)


def _clip_of(clip, what):
    """The C ABI's clip: the positive bound, or 0 for None (no inner clamp)."""
    if clip is None:
        return 0.0
    if isinstance(clip, bool) or not isinstance(clip, numbers.Real) or not math.isfinite(clip) or clip <= 0:
        raise ValueError(f"{what}={clip!r}: None (no clamp on the noise) or a positive finite number expected")
    return float(clip)


def _reduce_of(q_reduce):
    if q_reduce not in Q_REDUCE:
        raise ValueError(f"q_reduce={q_reduce!r}: 'first' (SB3's q1_forward), 'min' (DrQ-v2) or 'mean' expected")
    return q_reduce


def _noise_of(noise, sigma, B, A, device):
    """The (B, A) standard-normal tensor of a call, or None when nothing is added.  sigma == 0: none.  noise None: drawn on the device."""
    if sigma == 0.0:
        return None
    if noise is None:
        return torch.randn(B, A, dtype=torch.float32, device=device)
    if not isinstance(noise, torch.Tensor) or tuple(noise.shape) != (B, A):
        raise ValueError(f"noise: ({B}, {A}) expected, got {tuple(noise.shape) if isinstance(noise, torch.Tensor) else type(noise).__name__}")
    return H._rows(noise, "noise", A)


class TD3ActorFn(torch.autograd.Function):
    """(features (B, F), noise (B, A) or None, sigma, clip, arch, n, store, *actor parameters in actor_flat order) -> actions (B, A).  One launch;
    the backward (2 launches) returns d features and every actor gradient.  `store`: a backward may follow, so the forward gets a workspace;
    the actions have the same bits either way."""

    @staticmethod
    def forward(ctx, x, noise, sigma, clip, arch, n, store, *params):
        B, A = x.shape[0], arch[1]
        flat = [_dev(t) for t in params]
        lib = L.lib()
        d = _desc(arch, n, actor=flat)
        actions = torch.empty(B, A, dtype=torch.float32, device=x.device)
        ws = _ws(lib.m3l_td3_ws_bytes(C.byref(d), B), x.device) if store else None
        L.check(lib.m3l_td3_actor_fwd(C.byref(d), B, L.ptr(x), L.ptr(noise), sigma, clip, L.ptr(ws), L.ptr(actions), _stream()), "m3l_td3_actor_fwd")
        ctx.saved = (x, arch, n, flat, ws)
        return actions

    @staticmethod
    def backward(ctx, dactions):
        x, arch, n, flat, ws = ctx.saved
        if ws is None:
            raise H.no_workspace("TD3ActorFn")
        B = x.shape[0]
        da = _dev(dactions).reshape(B, arch[1])
        grads = [torch.empty_like(t) for t in flat]
        dx = torch.empty_like(x)
        d, gd = _desc(arch, n, actor=flat), _desc(arch, n, actor=grads)
        L.check(L.lib().m3l_td3_actor_bwd(C.byref(d), B, L.ptr(x), L.ptr(da), L.ptr(ws), L.ptr(dx), C.byref(gd), _stream()), "m3l_td3_actor_bwd")
        return (dx, None, None, None, None, None, None) + tuple(grads)


class TD3CriticLossFn(torch.autograd.Function):
    """(q (n, B), target_q (B,), weights (B,) or None, want_td) -> (sum_c mean(weights * (q_c - target_q)^2) 0-d, td_abs (B,) = the mean over the
    critics of |q_c - target_q|, no gradient; an empty tensor without want_td).  One launch each way; the gradient goes to q."""

    @staticmethod
    def forward(ctx, q, target_q, weights, want_td):
        n, B = q.shape
        loss = torch.empty((), dtype=torch.float32, device=q.device)
        coef = torch.empty(n, B, dtype=torch.float32, device=q.device)
        td_abs = torch.empty(B if want_td else 0, dtype=torch.float32, device=q.device)
        L.check(L.lib().m3l_td3_critic_loss_fwd(L.ptr(q), L.ptr(target_q), L.ptr(weights), n, B, L.ptr(loss), L.ptr(coef),
                                                L.ptr(td_abs) if want_td else None, _stream()), "m3l_td3_critic_loss_fwd")
        ctx.saved = coef
        ctx.mark_non_differentiable(td_abs)
        return loss, td_abs

    @staticmethod
    def backward(ctx, dloss, _dtd):
        coef = ctx.saved
        return H.scale_coef(dloss, coef), None, None, None


class TD3ActorLossFn(torch.autograd.Function):
    """(q (n, B), reduce 0 = min / 1 = mean) -> -mean(reduce_c q_c), 0-d.  One launch each way; the gradient goes to q."""

    @staticmethod
    def forward(ctx, q, reduce):
        n, B = q.shape
        loss = torch.empty((), dtype=torch.float32, device=q.device)
        coef = torch.empty(n, B, dtype=torch.float32, device=q.device)
        L.check(L.lib().m3l_td3_actor_loss_fwd(L.ptr(q), n, B, reduce, L.ptr(loss), L.ptr(coef), _stream()), "m3l_td3_actor_loss_fwd")
        ctx.saved = coef
        return loss

    @staticmethod
    def backward(ctx, dloss):
        coef = ctx.saved
        return H.scale_coef(dloss, coef), None


def actions(params: TD3Params, features, noise=None, noise_std=0.0, noise_clip=None):
    """actions (B, A) = smooth(mu(features), noise, noise_std, noise_clip); differentiable in the features and the actor's parameters.  Under
    `no_grad`, or when nothing requires a gradient, no workspace is sized or stored.  noise: (B, A) standard-normal draws; None with noise_std > 0: drawn on the device."""
    sigma, clip = _sigma_of(noise_std, "noise_std"), _clip_of(noise_clip, "noise_clip")
    flat = params.actor_flat()
    H.require_params(flat, "TD3 head parameter")
    x = H.features_of(features, on_tape=True)
    arch = _arch(x.shape[1], params)
    noise = _noise_of(noise, sigma, x.shape[0], arch[1], x.device)
    store = torch.is_grad_enabled() and (x.requires_grad or any(t.requires_grad for t in flat))
    return TD3ActorFn.apply(x, noise, sigma, clip, arch, params.n_critics, store, *flat)


def q_values(params: TD3Params, features, actions, target=False, param_grads=True, critics=None):
    """q (N, B) of all critics (the target critics with target=True) at cat([features, actions]), by the ensemble's node; differentiable in the
    actions and, unless param_grads=False, the critics' parameters; the features enter detached.  critics=1: only critic 0, through a
    one-critic descriptor -> q (1, B)."""
    n = params.n_critics if critics is None else int(critics)
    flat = params.critic_flat(target)
    H.require_params(flat, "TD3 head parameter")
    x = H.features_of(features, on_tape=False)
    arch = _arch(x.shape[1], params)
    flat = flat[:2 * n * (len(arch[3]) + 1)]
    a = H.actions_of(actions, x.shape[0], arch[1])
    want = param_grads and any(t.requires_grad for t in flat)
    store = torch.is_grad_enabled() and (a.requires_grad or want)
    return SE.SACEnsCriticFn.apply(x, a, arch, n, store, want, *flat)


@torch.no_grad()
def td_target(params: TD3Params, next_features, rewards, dones, gamma, noise=None, target_policy_noise=0.2, target_noise_clip=0.5,
              use_actor_target=True):
    """target_q (B,) = r + (1 - done) * gamma * min_c q_target_c(x', a'), a' = smooth(mu_target(x'), noise, target_policy_noise,
    target_noise_clip).  One launch, no tape.  gamma: a number, or one discount per row as `m3l_amd.sac.td_target` takes it (the `discounts` of
    an n-step batch).  noise None: a standard normal drawn on the device.  use_actor_target=False: the online actor proposes a' (DrQ-v2)."""
    sigma, clip = _sigma_of(target_policy_noise, "target_policy_noise"), _clip_of(target_noise_clip, "target_noise_clip")
    af, cf = params.actor_flat(bool(use_actor_target)), params.critic_flat(True)
    H.require_params(af + cf, "TD3 head parameter")
    x = H.features_of(next_features, on_tape=False)
    arch = _arch(x.shape[1], params)
    B = x.shape[0]
    noise = _noise_of(noise, sigma, B, arch[1], x.device)
    r, dn = _vec(rewards, "rewards", B), _vec(dones, "dones", B)
    per_row, gamma = _gamma_of(gamma, B)
    af, cf = [_dev(t) for t in af], [_dev(t) for t in cf]
    d = _desc(arch, params.n_critics, actor=af, critic=cf)
    out = torch.empty(B, dtype=torch.float32, device=x.device)
    L.check(L.lib().m3l_td3_td_target(C.byref(d), B, L.ptr(x), L.ptr(noise), sigma, clip, L.ptr(r), L.ptr(dn), L.ptr(gamma) if per_row else None,
                                      0.0 if per_row else gamma, L.ptr(out), _stream()), "m3l_td3_td_target")
    return out


def critic_loss_from(q, target_q, weights=None, return_td_errors=False):
    """sum_c mean(weights * (q_c - target_q)^2) from q (N, B) of `q_values`; weights (B,) or (B, 1) float32 or None (ones).
    return_td_errors: (loss, td) with td (B,) the mean over the critics of |q_c - target_q|, detached: what `update_priorities` takes."""
    q, _, B = SE._q_of(q)
    weights = H.weights_of(weights, B)
    loss, td = TD3CriticLossFn.apply(q, _vec(target_q, "target_q", B), weights, bool(return_td_errors))
    return (loss, td) if return_td_errors else loss


def actor_loss_from(q, q_reduce="first"):
    """-mean(reduce_c q_c) from q of `q_values`: (1, B) for "first", (N, B) for "min" and "mean"."""
    name = _reduce_of(q_reduce)
    q, n, _ = SE._q_of(q)
    if name == "first" and n != 1:
        raise ValueError(f"q_reduce='first' takes q (1, B) of critic 0 alone (q_values(..., critics=1)), got {tuple(q.shape)}")
    return TD3ActorLossFn.apply(q, Q_REDUCE[name])


class _Actor(nn.Module):
    def __init__(self, features_dim, pi, action_dim):
        super().__init__()
        k = pi[-1] if pi else features_dim
        self.mu = nn.Sequential(*H.mlp(features_dim, pi, nn.ReLU), nn.Linear(k, action_dim), nn.Tanh())


class TD3Head(nn.Module):
    """The parameters of SB3's `TD3Policy` behind the features extractor under its names (`actor.mu.{0,2,..}`, `actor_target.mu.*`,
    `critic.qf{i}.*`, `critic_target.qf{i}.*`), so that part of an SB3 policy's state dict loads with strict=True, and the head's part of a TD3,
    DDPG (`n_critics=1`) or DrQ-v2 gradient step on the HIP kernels.  Both targets start as copies and take no gradient.  `policy_delay` and
    every noise schedule belong to the caller's loop.  Parity with SB3 is unpinned (SB3 is not in the reference tree)."""

    def __init__(self, features_dim, action_dim, net_arch=None, n_critics=2, activation_fn=nn.ReLU, share_features_extractor=True):
        super().__init__()
        if activation_fn is not nn.ReLU:
            raise ValueError(f"activation_fn={getattr(activation_fn, '__name__', activation_fn)}: the HIP TD3 head computes ReLU only")
        self.share_features_extractor = bool(share_features_extractor)
        H.require_shared_extractor(self, "TD3")
        self.n_critics = SE._n_critics_of(n_critics)
        try:
            self.features_dim, self.action_dim, pi, qf = H.head_dims(features_dim, action_dim, net_arch, [256, 256], "qf", "TD3", "net")
        except ValueError as e:
            if str(e).startswith("width "):
                raise ValueError(f"{e}; SB3's own TD3 default net_arch=[400, 300] is outside that rule (300 is not a multiple of 16): use "
                                 "[256, 256], the default here") from None
            raise
        self.actor = _Actor(self.features_dim, pi, self.action_dim)
        self.actor_target = _Actor(self.features_dim, pi, self.action_dim)
        self.actor_target.load_state_dict(self.actor.state_dict())
        self.actor_target.requires_grad_(False)
        self.critic = SE._Critic(self.features_dim, qf, self.action_dim, self.n_critics)
        self.critic_target = SE._Critic(self.features_dim, qf, self.action_dim, self.n_critics)
        self.critic_target.load_state_dict(self.critic.state_dict())
        self.critic_target.requires_grad_(False)

    def params(self) -> TD3Params:
        return TD3Params.from_policy(self)

    @torch.no_grad()
    def forward(self, features, noise=None, noise_std=0.0, noise_clip=None):
        """actions (B, A), no gradient: SB3's `_predict` after `extract_features`, with the exploration noise when noise_std > 0."""
        return actions(self.params(), features, noise, noise_std, noise_clip)

    def actions(self, features, noise=None, noise_std=0.0, noise_clip=None):
        return actions(self.params(), features, noise, noise_std, noise_clip)

    def q_values(self, features, actions, target=False):
        return q_values(self.params(), features, actions, target)

    def td_target(self, next_features, rewards, dones, gamma, noise=None, target_policy_noise=0.2, target_noise_clip=0.5, use_actor_target=True):
        return td_target(self.params(), next_features, rewards, dones, gamma, noise, target_policy_noise, target_noise_clip, use_actor_target)

    def critic_loss(self, features, actions, target_q, weights=None, return_td_errors=False):
        """sum_c mean(weights * (q_c(features, actions) - target_q)^2), and the td errors for `update_priorities` when asked for."""
        with torch.no_grad():
            a = actions.detach()
        return critic_loss_from(q_values(self.params(), features, a), target_q, weights, return_td_errors)

    def actor_loss(self, features, q_reduce="first", noise=None, noise_std=0.0, noise_clip=None):
        """-mean(reduce_c q_c(features, actions(features))).  "first" evaluates critic 0 alone.  The critics give their gradient in the actions
        only: their parameters receive nothing from this loss."""
        name = _reduce_of(q_reduce)
        p = self.params()
        a = actions(p, features, noise, noise_std, noise_clip)
        q = q_values(p, features, a, param_grads=False, critics=1 if name == "first" else None)
        return actor_loss_from(q, name)

    @torch.no_grad()
    def polyak_update(self, tau):
        """target = (1 - tau) * target + tau * online over every tensor of the critics and of the actor, one multi-tensor launch per net."""
        update_moving_average(self.critic_target, self.critic, 1.0 - float(tau))
        update_moving_average(self.actor_target, self.actor, 1.0 - float(tau))
