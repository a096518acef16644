"""The SAC policy head on the HIP kernels of m3l_amd/csrc/sac.hip: everything between the extractor's features and the three optimizers in one
gradient step of `SAC_MAE.train` (`models/sac_mae.py:303-366`), and the actor on every environment step.

  head  : Stable-Baselines3's `SACPolicy` as `MAESACPolicy` configures it (`nn.ReLU`, `n_critics=2`, `share_features_extractor=True`,
          `use_sde=False`): `actor.latent_pi` of Linear + ReLU, `actor.mu`, a state-dependent `actor.log_std` clamped to [-20, 2], the
          tanh-squashed Gaussian, and twin critics `qf0` / `qf1` over cat([features, actions]).  SB3 is not part of the reference tree:
          PARITY UNPINNED for its arithmetic, as for vit-pytorch and the PPO head; tests/sac_cases.py restates it from torch primitives.
  step  : the reference's own lines: the entropy-coefficient loss (:311-312), the TD target (:326-335), the critic loss (:339-342), the actor
          loss (:354-356) and the Polyak update (:365-366).
  nodes : `SACActorFn` (1 launch forward, 2 backward), `SACCriticFn` (1 forward, 1 or 2 backward) and one node per loss (1 + 1).  `td_target`
          is one launch without a tape.  The entropy coefficient travels as a float or as the device tensor `log_ent_coef`, whose exp the
          kernels take: a step reads nothing back to the host (the reference reads four values).

The features enter the critics detached (the extractor is shared, as in SB3), and `actor_loss` takes the critics' gradient in the actions only:
the critic's parameters get nothing from it.  The reference lets `actor_loss.backward()` fill those `.grad`s and discards them at the next
`critic.optimizer.zero_grad()` (:347).  Everything is float32; there is no eager fallback.
"""
import ctypes as C
import numbers
from typing import NamedTuple, Tuple

import torch
from torch import nn

from . import _head as H
from . import _lib as L
from ._head import _dev, _vec
from .dino import update_moving_average
from .functional import _require_cuda, _stream, _ws

LOG_STD_MIN, LOG_STD_MAX = -20.0, 2.0
MAX_CRITICS = L.SAC_MAX_CRITICS          # of a SACEnsembleHead (sac_ensemble.py); a SACHead has exactly 2
WB = Tuple[torch.Tensor, torch.Tensor]


class SACHeadParams(NamedTuple):
    """The parameter tensors of a head, torch.nn.Linear layouts.  pi: (weight, bias) per hidden layer of latent_pi; qf / qf_target: per critic,
    (weight, bias) of every Linear, the last one being the Linear(., 1)."""
    pi: Tuple[WB, ...]
    mu: WB
    log_std: WB
    qf: Tuple[Tuple[WB, ...], Tuple[WB, ...]]
    qf_target: Tuple[Tuple[WB, ...], Tuple[WB, ...]]

    def actor_flat(self):
        return [t for wb in self.pi for t in wb] + list(self.mu) + list(self.log_std)

    def critic_flat(self, target=False):
        return [t for net in (self.qf_target if target else self.qf) for wb in net for t in wb]

    @staticmethod
    def from_policy(policy) -> "SACHeadParams":
        """From a module with SB3's attribute names (`actor.latent_pi / mu / log_std`, `critic.qf0 / qf1`, `critic_target.qf0 / qf1`): a `SACHead`,
        or an SB3 `SACPolicy`, whose configuration is checked against what the kernels compute."""
        _reject_sac_flags(policy)
        for name, c in (("critic", policy.critic), ("critic_target", policy.critic_target)):
            n = getattr(c, "n_critics", 2)
            if n != 2 or hasattr(c, "qf2") or not hasattr(c, "qf1"):
                raise ValueError(f"{name}: n_critics={n if n != 2 else 'other than 2'}: the HIP SAC head computes exactly 2 critics")
        return SACHeadParams(*_read_policy(policy, 2))


def _read_policy(policy, n_critics):
    """(pi, mu, log_std, qf, qf_target) of a module with SB3's attribute names and `n_critics` critics `qf0 ..`, its actor and extractor sharing
    checked against what the kernels compute; the caller has checked the critic count."""
    actor, critic, target = policy.actor, policy.critic, policy.critic_target
    if getattr(actor, "use_sde", False):
        raise ValueError("use_sde=True (generalised state-dependent exploration) is not computed by the HIP SAC head")
    if not isinstance(getattr(actor, "log_std", None), nn.Linear):
        raise ValueError("actor.log_std is not an nn.Linear: the HIP SAC head computes a state-dependent log_std (use_sde=False) only")
    for c in (critic, target):
        H.require_shared_extractor(c, "SAC")
    pi = H.linear_pairs(actor.latent_pi, "actor.latent_pi", nn.ReLU, "SAC")
    qf = tuple(_q_net(getattr(critic, f"qf{i}"), f"critic.qf{i}") for i in range(n_critics))
    qt = tuple(_q_net(getattr(target, f"qf{i}"), f"critic_target.qf{i}") for i in range(n_critics))
    return pi, (actor.mu.weight, actor.mu.bias), (actor.log_std.weight, actor.log_std.bias), qf, qt


def _q_net(seq, name):
    mods = list(seq)
    if not mods or not isinstance(mods[-1], nn.Linear) or mods[-1].bias is None or mods[-1].out_features != 1:
        raise ValueError(f"{name}: a net ending in nn.Linear(., 1) with a bias expected")
    return H.linear_pairs(mods[:-1], name, nn.ReLU, "SAC") + ((mods[-1].weight, mods[-1].bias),)


def _reject_flags(policy):
    if getattr(policy, "use_sde", False):
        raise ValueError("use_sde=True (generalised state-dependent exploration) is not computed by the HIP SAC head")
    H.require_shared_extractor(policy, "SAC")


def _reject_sac_flags(policy):
    _reject_flags(policy)
    n = getattr(policy, "n_critics", 2)
    if n != 2:
        raise ValueError(f"n_critics={n}: the HIP SAC head computes exactly 2 critics")


def _arch(F, params):
    """(F, A, pi widths, qf widths) with every shape checked; raises ValueError for a head outside the kernels' limits.  params: SACHeadParams
    (exactly 2 critics), or the SACEnsembleParams of sac_ensemble.py (1 to MAX_CRITICS, as many targets)."""
    F = int(F)
    A = int(params.mu[0].shape[0])
    H.check_float32(params.actor_flat() + params.critic_flat() + params.critic_flat(True), "SAC")
    k, pi = H.layer_widths(F, params.pi, "pi", "SAC", "net")
    H.check_head_linear("mu", params.mu, A, k)
    H.check_head_linear("log_std", params.log_std, A, k)
    twin = isinstance(params, SACHeadParams)
    qf = None
    for stem, nets in (("qf", params.qf), ("qf_target", params.qf_target)):
        if twin and len(nets) != 2:
            raise ValueError(f"{stem}: {len(nets)} critics: the HIP SAC head computes exactly 2 critics")
        if not twin and (not 1 <= len(nets) <= MAX_CRITICS or len(nets) != len(params.qf)):
            raise ValueError(f"{stem}: {len(nets)} critics: the HIP SAC critic ensemble computes 1 to {MAX_CRITICS} critics and as many targets")
        for i, net in enumerate(nets):
            name = f"{stem}{i}"
            k, ws = H.layer_widths(F + A, net[:-1], name, "SAC", "net")
            for w, b in net[-1:]:          # the Linear(., 1) on top
                if tuple(w.shape) != (1, k) or tuple(b.shape) != (1,):
                    raise ValueError(f"{name} layer {len(net) - 1}: weight {tuple(w.shape)} / bias {tuple(b.shape)} do not follow an input of width {k}")
            if qf is not None and ws != qf:
                raise ValueError(f"{name}: hidden widths {ws}, the other critics have {qf}: the {'two' if twin else len(params.qf)} critics and their "
                                 "targets must be alike")
            qf = ws
    H.check_limits((F,) + pi + qf, A)
    return F, A, pi, qf


def _desc(arch, actor=None, critic=None):
    """m3l_sac_desc over the tensors of `actor` (SACHeadParams.actor_flat order) and / or `critic` (critic_flat order); the caller keeps them alive."""
    F, A, pi, qf = arch
    d = L.SacDesc()
    d.features, d.actions, d.n_pi, d.n_qf = F, A, len(pi), len(qf)
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
        for c in range(2):
            for l in range(len(qf)):
                d.qf_weight[c][l], d.qf_bias[c][l] = next(it).data_ptr(), next(it).data_ptr()
            d.q_weight[c], d.q_bias[c] = next(it).data_ptr(), next(it).data_ptr()
    return d


class SACActorFn(torch.autograd.Function):
    """(features (B, F), noise (B, A) or None, arch, store, *actor parameters in actor_flat order) -> actions (B, A), log_prob (B,).  One launch;
    the backward (2 launches) returns d features and every actor gradient.  `store` as in ActorCriticEvalFn: a backward may follow, so the
    forward gets a workspace; the outputs have the same bits either way."""

    @staticmethod
    def forward(ctx, x, noise, arch, store, *params):
        B, A = x.shape[0], arch[1]
        flat = [_dev(t) for t in params]
        lib = L.lib()
        d = _desc(arch, actor=flat)
        actions = torch.empty(B, A, dtype=torch.float32, device=x.device)
        logp = torch.empty(B, dtype=torch.float32, device=x.device)
        ws = _ws(lib.m3l_sac_ws_bytes(C.byref(d), B), x.device) if store else None
        L.check(lib.m3l_sac_actor_fwd(C.byref(d), B, L.ptr(x), L.ptr(noise), L.ptr(ws), L.ptr(actions), L.ptr(logp), _stream()), "m3l_sac_actor_fwd")
        ctx.saved = (x, noise, arch, flat, ws)
        ctx.set_materialize_grads(False)
        return actions, logp

    @staticmethod
    def backward(ctx, dactions, dlogp):
        x, noise, arch, flat, ws = ctx.saved
        if ws is None:
            raise H.no_workspace("SACActorFn")
        B = x.shape[0]
        da = None if dactions is None else _dev(dactions).reshape(B, arch[1])
        dl = None if dlogp is None else _dev(dlogp).reshape(B)
        grads = [torch.empty_like(t) for t in flat]
        dx = torch.empty_like(x)
        d, gd = _desc(arch, actor=flat), _desc(arch, actor=grads)
        L.check(L.lib().m3l_sac_actor_bwd(C.byref(d), B, L.ptr(x), L.ptr(noise), L.ptr(da), L.ptr(dl), L.ptr(ws), L.ptr(dx), C.byref(gd), _stream()),
                "m3l_sac_actor_bwd")
        return (dx, None, None, None) + tuple(grads)


class SACCriticFn(torch.autograd.Function):
    """(features (B, F), actions (B, A), arch, store, param_grads, *critic parameters in critic_flat order) -> q (2, B).  One launch.  The backward
    returns d actions (1 launch) and, with param_grads, every critic gradient (1 more); the features never take a gradient."""

    @staticmethod
    def forward(ctx, x, actions, arch, store, param_grads, *params):
        B = x.shape[0]
        flat = [_dev(t) for t in params]
        lib = L.lib()
        d = _desc(arch, critic=flat)
        q = torch.empty(2, B, dtype=torch.float32, device=x.device)
        ws = _ws(lib.m3l_sac_ws_bytes(C.byref(d), B), x.device) if store else None
        L.check(lib.m3l_sac_critic_fwd(C.byref(d), B, L.ptr(x), L.ptr(actions), L.ptr(ws), L.ptr(q), _stream()), "m3l_sac_critic_fwd")
        ctx.saved = (arch, flat, ws, B, bool(param_grads))
        return q

    @staticmethod
    def backward(ctx, dq):
        arch, flat, ws, B, param_grads = ctx.saved
        if ws is None:
            raise H.no_workspace("SACCriticFn")
        dq = _dev(dq).reshape(2, B)
        dactions = torch.empty(B, arch[1], dtype=torch.float32, device=dq.device) if ctx.needs_input_grad[1] else None
        grads = [torch.empty_like(t) for t in flat] if param_grads else None
        d = _desc(arch, critic=flat)
        gd = C.byref(_desc(arch, critic=grads)) if param_grads else None
        L.check(L.lib().m3l_sac_critic_bwd(C.byref(d), B, L.ptr(dq), L.ptr(ws), L.ptr(dactions), gd, _stream()), "m3l_sac_critic_bwd")
        return (None, dactions, None, None, None) + (tuple(grads) if param_grads else (None,) * len(flat))


class SACCriticLossFn(torch.autograd.Function):
    """(q (2, B), target_q (B,)) -> 0.5 * sum_c mse(q_c, target_q), 0-d (`sac_mae.py:342`).  One launch each way; the gradient goes to q."""

    @staticmethod
    def forward(ctx, q, target_q):
        B = target_q.numel()
        loss = torch.empty((), dtype=torch.float32, device=q.device)
        coef = torch.empty(2, B, dtype=torch.float32, device=q.device)
        L.check(L.lib().m3l_sac_critic_loss_fwd(L.ptr(q), L.ptr(target_q), B, L.ptr(loss), L.ptr(coef), _stream()), "m3l_sac_critic_loss_fwd")
        ctx.saved = (coef, B)
        return loss

    @staticmethod
    def backward(ctx, dloss):
        coef, B = ctx.saved
        dq = torch.empty_like(coef)
        L.check(L.lib().m3l_sac_critic_loss_bwd(L.ptr(_dev(dloss)), L.ptr(coef), B, L.ptr(dq), _stream()), "m3l_sac_critic_loss_bwd")
        return dq, None


class SACCriticLossWFn(torch.autograd.Function):
    """(q (2, B), target_q (B,), weights (B,) or None) -> (0.5 * sum_c mean(weights * (q_c - target_q)^2) 0-d, td_abs (B,) = the mean over the two
    critics of |q_c - target_q|, no gradient): the critic loss under the importance weights of prioritised replay, and what
    `update_priorities` takes.  One launch each way (m3l_sac_critic_loss_w_fwd, m3l_sac_critic_loss_bwd); the gradient goes to q."""

    @staticmethod
    def forward(ctx, q, target_q, weights):
        B = target_q.numel()
        loss = torch.empty((), dtype=torch.float32, device=q.device)
        coef = torch.empty(2, B, dtype=torch.float32, device=q.device)
        td_abs = torch.empty(B, dtype=torch.float32, device=q.device)
        L.check(L.lib().m3l_sac_critic_loss_w_fwd(L.ptr(q), L.ptr(target_q), L.ptr(weights), B, L.ptr(loss), L.ptr(coef), L.ptr(td_abs), _stream()),
                "m3l_sac_critic_loss_w_fwd")
        ctx.saved = (coef, B)
        ctx.mark_non_differentiable(td_abs)
        return loss, td_abs

    @staticmethod
    def backward(ctx, dloss, _dtd):
        coef, B = ctx.saved
        dq = torch.empty_like(coef)
        L.check(L.lib().m3l_sac_critic_loss_bwd(L.ptr(_dev(dloss)), L.ptr(coef), B, L.ptr(dq), _stream()), "m3l_sac_critic_loss_bwd")
        return dq, None, None


class SACActorLossFn(torch.autograd.Function):
    """(log_prob (B,), q (2, B), ent_coef float or None, log_ent_coef tensor or None) -> mean(ent_coef * log_prob - min_c q_c), 0-d
    (`sac_mae.py:354-356`).  One launch each way; the gradient goes to log_prob and q, the entropy coefficient is a constant (:311)."""

    @staticmethod
    def forward(ctx, logp, q, ent_coef, log_ent_coef):
        B = logp.numel()
        loss = torch.empty((), dtype=torch.float32, device=q.device)
        coef = torch.empty(3, B, dtype=torch.float32, device=q.device)
        L.check(L.lib().m3l_sac_actor_loss_fwd(L.ptr(logp), L.ptr(q), B, 0.0 if ent_coef is None else float(ent_coef), L.ptr(log_ent_coef), L.ptr(loss),
                                               L.ptr(coef), _stream()), "m3l_sac_actor_loss_fwd")
        ctx.saved = (coef, B)
        return loss

    @staticmethod
    def backward(ctx, dloss):
        coef, B = ctx.saved
        out = torch.empty_like(coef)
        L.check(L.lib().m3l_sac_actor_loss_bwd(L.ptr(_dev(dloss)), L.ptr(coef), B, L.ptr(out), _stream()), "m3l_sac_actor_loss_bwd")
        return out[0], out[1:], None, None


class SACEntCoefLossFn(torch.autograd.Function):
    """(log_ent_coef (1,), log_prob (B,), target_entropy) -> loss 0-d = -mean(log_ent_coef * (log_prob + target_entropy)), ent_coef 0-d =
    exp(log_ent_coef) (no gradient) (`sac_mae.py:311-312`).  One launch each way; the gradient goes to log_ent_coef."""

    @staticmethod
    def forward(ctx, log_ent_coef, logp, target_entropy):
        B = logp.numel()
        loss = torch.empty((), dtype=torch.float32, device=logp.device)
        ent = torch.empty((), dtype=torch.float32, device=logp.device)
        L.check(L.lib().m3l_sac_ent_coef_loss(L.ptr(log_ent_coef), L.ptr(logp), float(target_entropy), B, None, L.ptr(loss), L.ptr(ent), None, _stream()),
                "m3l_sac_ent_coef_loss")
        ctx.saved = (log_ent_coef, logp, float(target_entropy), B)
        ctx.mark_non_differentiable(ent)
        return loss, ent

    @staticmethod
    def backward(ctx, dloss, _dent):
        log_ent_coef, logp, target_entropy, B = ctx.saved
        g = torch.empty_like(log_ent_coef)
        L.check(L.lib().m3l_sac_ent_coef_loss(L.ptr(log_ent_coef), L.ptr(logp), target_entropy, B, L.ptr(_dev(dloss)), None, None, L.ptr(g), _stream()),
                "m3l_sac_ent_coef_loss")
        return g, None, None


def _ent_args(ent_coef, log_ent_coef):
    """(float or None, device tensor or None): exactly one of the two forms."""
    if (ent_coef is None) == (log_ent_coef is None):
        raise ValueError("give the entropy coefficient either as ent_coef (a number) or as log_ent_coef (a device tensor), one of the two")
    if log_ent_coef is not None:
        _require_cuda(log_ent_coef, "log_ent_coef")
        if log_ent_coef.numel() != 1 or log_ent_coef.dtype != torch.float32:
            raise ValueError(f"log_ent_coef: one float32 value expected, got {tuple(log_ent_coef.shape)} {log_ent_coef.dtype}")
        return None, log_ent_coef.detach()
    if isinstance(ent_coef, torch.Tensor):
        raise ValueError("ent_coef is a number; pass a tensor as log_ent_coef (its exp is taken on the device)")
    return float(ent_coef), None


def action_log_prob(params: SACHeadParams, features, noise=None, deterministic=False):
    """actions (B, A) = tanh(mu + exp(log_std) * noise), log_prob (B,); differentiable in the features and the actor's parameters.  Under `no_grad`,
    or when nothing requires a gradient, no workspace is allocated and nothing is stored."""
    flat = params.actor_flat()
    H.require_params(flat, "SAC head parameter")
    x = H.features_of(features, on_tape=True)
    arch = _arch(x.shape[1], params)
    noise = H.noise_of(noise, x.shape[0], arch[1], x.device, deterministic)
    store = torch.is_grad_enabled() and (x.requires_grad or any(t.requires_grad for t in flat))
    return SACActorFn.apply(x, noise, arch, store, *flat)


def q_values(params: SACHeadParams, features, actions, target=False, param_grads=True):
    """q (2, B) of both critics (the target critics with target=True) at cat([features, actions]); differentiable in the actions and, unless
    param_grads=False, the critic's parameters; the features enter detached."""
    flat = params.critic_flat(target)
    H.require_params(flat, "SAC head parameter")
    x = H.features_of(features, on_tape=False)
    arch = _arch(x.shape[1], params)
    a = H.actions_of(actions, x.shape[0], arch[1])
    want = param_grads and any(t.requires_grad for t in flat)
    store = torch.is_grad_enabled() and (a.requires_grad or want)
    return SACCriticFn.apply(x, a, arch, store, want, *flat)


def _gamma_of(gamma, B):
    """(True, discounts (B,) on the device) for a tensor of one discount per row, (False, the number) otherwise."""
    if isinstance(gamma, torch.Tensor):
        _require_cuda(gamma, "gamma")
        if gamma.dtype != torch.float32 or tuple(gamma.shape) not in ((B,), (B, 1)):
            raise ValueError(f"gamma: a number, or a float32 tensor of shape ({B},) or ({B}, 1), one discount per row; got {tuple(gamma.shape)} "
                             f"{gamma.dtype}")
        return True, _vec(gamma, "gamma", B)
    if not isinstance(gamma, numbers.Real):
        raise ValueError(f"gamma: a number or a float32 CUDA tensor of {B} values expected, got {type(gamma).__name__}")
    return False, float(gamma)


@torch.no_grad()
def td_target(params: SACHeadParams, next_features, rewards, dones, gamma, ent_coef=None, log_ent_coef=None, noise=None):
    """target_q (B,) = r + (1 - done) * gamma * (min_c q_target_c(x', a') - ent_coef * logp') with (a', logp') = actor(x') (`sac_mae.py:326-335`).
    One launch, no tape.  gamma: a Python number, or a float32 CUDA tensor of B values, (B,) or (B, 1): one discount per row, the `discounts` of
    an n-step batch (m3l_sac_td_target_rows; a constant tensor gives the bits of the number)."""
    af, cf = params.actor_flat(), params.critic_flat(True)
    H.require_params(af + cf, "SAC head parameter")
    x = H.features_of(next_features, on_tape=False)
    arch = _arch(x.shape[1], params)
    B = x.shape[0]
    noise = H.noise_of(noise, B, arch[1], x.device)
    ent, log_ent = _ent_args(ent_coef, log_ent_coef)
    r, dn = _vec(rewards, "rewards", B), _vec(dones, "dones", B)
    per_row, gamma = _gamma_of(gamma, B)
    af, cf = [_dev(t) for t in af], [_dev(t) for t in cf]
    d = _desc(arch, actor=af, critic=cf)
    out = torch.empty(B, dtype=torch.float32, device=x.device)
    if per_row:
        L.check(L.lib().m3l_sac_td_target_rows(C.byref(d), B, L.ptr(x), L.ptr(noise), L.ptr(r), L.ptr(dn), L.ptr(gamma), 0.0 if ent is None else ent,
                                               L.ptr(log_ent), L.ptr(out), _stream()), "m3l_sac_td_target_rows")
    else:
        L.check(L.lib().m3l_sac_td_target(C.byref(d), B, L.ptr(x), L.ptr(noise), L.ptr(r), L.ptr(dn), float(gamma), 0.0 if ent is None else ent,
                                          L.ptr(log_ent), L.ptr(out), _stream()), "m3l_sac_td_target")
    return out


def critic_loss_from(q, target_q, weights=None, return_td_errors=False):
    """0.5 * sum_c mse(q_c, target_q) from q (2, B) of `q_values`.  weights (B,) or (B, 1) float32, the importance weights of a
    `PrioritizedReplayBatch`: 0.5 * sum_c mean(weights * (q_c - target_q)^2).  return_td_errors: (loss, td) with td (B,) the mean over the two
    critics of |q_c - target_q|, detached: what `DeviceReplayBuffer.update_priorities` takes.  With neither, the unweighted entry runs."""
    _require_cuda(q, "q")
    B = q.shape[-1]
    if q.dim() != 2 or q.shape[0] != 2 or q.dtype != torch.float32:
        raise ValueError(f"q: (2, B) float32 expected, got {tuple(q.shape)} {q.dtype}")
    if weights is None and not return_td_errors:
        return SACCriticLossFn.apply(q.contiguous(), _vec(target_q, "target_q", B))
    weights = H.weights_of(weights, B)
    loss, td = SACCriticLossWFn.apply(q.contiguous(), _vec(target_q, "target_q", B), weights)
    return (loss, td) if return_td_errors else loss


def actor_loss_from(log_prob, q, ent_coef=None, log_ent_coef=None):
    """mean(ent_coef * log_prob - min_c q_c) from the outputs of `action_log_prob` and `q_values`."""
    _require_cuda(q, "q")
    _require_cuda(log_prob, "log_prob")
    B = q.shape[-1]
    if q.dim() != 2 or q.shape[0] != 2 or q.dtype != torch.float32 or log_prob.numel() != B or log_prob.dtype != torch.float32:
        raise ValueError(f"q (2, B) and log_prob (B,) float32 expected, got {tuple(q.shape)} {q.dtype} and {tuple(log_prob.shape)} {log_prob.dtype}")
    ent, log_ent = _ent_args(ent_coef, log_ent_coef)
    return SACActorLossFn.apply(log_prob.contiguous().reshape(B), q.contiguous(), ent, log_ent)


def ent_coef_loss(log_ent_coef, log_prob, target_entropy):
    """(loss, ent_coef) as 0-d device tensors: -mean(log_ent_coef * (log_prob + target_entropy)) with log_prob a constant, exp(log_ent_coef)."""
    _require_cuda(log_ent_coef, "log_ent_coef")
    if log_ent_coef.numel() != 1 or log_ent_coef.dtype != torch.float32:
        raise ValueError(f"log_ent_coef: one float32 value expected, got {tuple(log_ent_coef.shape)} {log_ent_coef.dtype}")
    return SACEntCoefLossFn.apply(log_ent_coef, _vec(log_prob, "log_prob", log_prob.numel()), float(target_entropy))


class _Actor(nn.Module):
    def __init__(self, features_dim, pi, action_dim):
        super().__init__()
        self.latent_pi = H.mlp(features_dim, pi, nn.ReLU)
        k = pi[-1] if pi else features_dim
        self.mu = nn.Linear(k, action_dim)
        self.log_std = nn.Linear(k, action_dim)
        self.use_sde = False


class _Critic(nn.Module):
    def __init__(self, features_dim, qf, action_dim):
        super().__init__()
        self.n_critics, self.share_features_extractor = 2, True
        for i in range(2):
            setattr(self, f"qf{i}", H.mlp(features_dim + action_dim, qf, nn.ReLU, out=1))


class SACHead(nn.Module):
    """The parameters of SB3's `SACPolicy` behind the features extractor, with its names and layouts (`actor.latent_pi.{0,2,..}`, `actor.mu`,
    `actor.log_std`, `critic.qf{0,1}.{0,2,..}`, `critic_target.qf{0,1}.{0,2,..}`), so that part of an SB3 policy's state dict loads with
    strict=True, and the head's part of `SAC_MAE.train` computed by the HIP kernels.  `critic_target` starts as a copy of `critic` and takes no
    gradient.  Initial values are torch's nn.Linear defaults, as SB3's SAC uses; parity with SB3 is unpinned (SB3 is not in the reference tree)."""

    def __init__(self, features_dim, action_dim, net_arch=None, n_critics=2, activation_fn=nn.ReLU, use_sde=False, share_features_extractor=True):
        super().__init__()
        if activation_fn is not nn.ReLU:
            raise ValueError(f"activation_fn={getattr(activation_fn, '__name__', activation_fn)}: the HIP SAC head computes ReLU only")
        self.use_sde, self.share_features_extractor, self.n_critics = bool(use_sde), bool(share_features_extractor), n_critics
        _reject_sac_flags(self)
        self.features_dim, self.action_dim, pi, qf = H.head_dims(features_dim, action_dim, net_arch, [256, 256], "qf", "SAC", "net")
        action_dim = self.action_dim
        self.actor = _Actor(self.features_dim, pi, action_dim)
        self.critic = _Critic(self.features_dim, qf, action_dim)
        self.critic_target = _Critic(self.features_dim, qf, action_dim)
        self.critic_target.load_state_dict(self.critic.state_dict())
        self.critic_target.requires_grad_(False)

    def params(self) -> SACHeadParams:
        return SACHeadParams.from_policy(self)

    @torch.no_grad()
    def forward(self, features, deterministic=False, noise=None):
        """actions (B, A), no gradient: SB3's `_predict` after `extract_features`."""
        return action_log_prob(self.params(), features, noise, deterministic)[0]

    def action_log_prob(self, features, noise=None):
        return action_log_prob(self.params(), features, noise)

    def q_values(self, features, actions, target=False):
        return q_values(self.params(), features, actions, target)

    def td_target(self, next_features, rewards, dones, gamma, ent_coef=None, log_ent_coef=None, noise=None):
        return td_target(self.params(), next_features, rewards, dones, gamma, ent_coef, log_ent_coef, noise)

    def critic_loss(self, features, actions, target_q, weights=None, return_td_errors=False):
        """0.5 * sum_c mse(q_c(features, actions), target_q): 2 launches forward, 3 backward.  weights / return_td_errors: the importance
        weights of prioritised replay and the td errors for `update_priorities`, as `critic_loss_from` takes and returns them."""
        with torch.no_grad():
            a = actions.detach()
        return critic_loss_from(q_values(self.params(), features, a), target_q, weights, return_td_errors)

    def actor_loss(self, features, ent_coef=None, log_ent_coef=None, noise=None):
        """(loss, log_prob.detach()): mean(ent_coef * log_prob - min_c q_c(features, a_pi)).  The critics give their gradient in the actions only:
        their parameters receive nothing from this loss."""
        p = self.params()
        a_pi, logp = action_log_prob(p, features, noise)
        q = q_values(p, features, a_pi, param_grads=False)
        return actor_loss_from(logp, q, ent_coef, log_ent_coef), logp.detach()

    def ent_coef_loss(self, log_ent_coef, log_prob, target_entropy):
        return ent_coef_loss(log_ent_coef, log_prob, target_entropy)

    @torch.no_grad()
    def polyak_update(self, tau):
        """critic_target = (1 - tau) * critic_target + tau * critic over every tensor, in one multi-tensor launch (`sac_mae.py:366`)."""
        update_moving_average(self.critic_target, self.critic, 1.0 - float(tau))
