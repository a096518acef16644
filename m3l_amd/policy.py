"""The PPO policy head on the HIP kernels of m3l_amd/csrc/policy.hip: the arithmetic between the extractor's features and the scalar that
`PPO_MAE.train` calls backward on (`models/ppo_mae.py:280-340`), and the same head on every environment step (`MAEPolicy.forward`,
`models/pretrain_models.py:899-923`).

  head  : Stable-Baselines3's `ActorCriticPolicy` with `net_arch = dict(pi=[...], vf=[...])` and Tanh (`train.py:166`): two branches of
          Linear + Tanh, `action_net`, `value_net`, a state-independent `log_std`, the diagonal Gaussian's log-probability and entropy.
          SB3's `MlpExtractor`, `DiagGaussianDistribution` and `evaluate_actions` are not part of the reference tree: PARITY UNPINNED for
          them, as for vit-pytorch; tests/ppo_cases.py restates them from torch primitives.
  loss  : the reference's own lines (`ppo_mae.py:281-331`): advantage normalisation, clipped surrogate, optional value clipping, entropy
          term, and the five logged statistics, which stay on the device (one copy reads them, `PPOStats.stats_dict`).
  nodes : `ActorCriticEvalFn` (1 launch forward, 2 backward) and `PPOLossFn` (1 + 1), one autograd node each; the workspace of the
          forward is kept for the backward.  `act` is one launch and stores nothing for a backward.

Everything is float32 whatever the encoder's compute type: the ratio exp(logp - logp_old) is what PPO clips on.  There is no eager
fallback: every number comes from a kernel, torch owns memory and the autograd tape.
"""
import ctypes as C
from typing import NamedTuple, Tuple

import torch
from torch import nn

from . import _head as H
from . import _lib as L
from ._head import MAX_ACTIONS, MAX_HIDDEN, MAX_WIDTH, _dev, _rows, _vec  # noqa: F401  (the limits and the tensor preparation, under their names here)
from .functional import _require_cuda, _stream, _ws

STAT_NAMES = ("policy_loss", "value_loss", "entropy_loss", "clip_fraction", "approx_kl")


class HeadParams(NamedTuple):
    """The parameter tensors of a head, torch.nn.Linear layouts: pi / vf are tuples of (weight [out, in], bias [out]) per hidden layer."""
    pi: Tuple[Tuple[torch.Tensor, torch.Tensor], ...]
    vf: Tuple[Tuple[torch.Tensor, torch.Tensor], ...]
    action: Tuple[torch.Tensor, torch.Tensor]
    value: Tuple[torch.Tensor, torch.Tensor]
    log_std: torch.Tensor

    def flat(self):
        return [t for wb in self.pi for t in wb] + [t for wb in self.vf for t in wb] + list(self.action) + list(self.value) + [self.log_std]

    @staticmethod
    def from_policy(policy) -> "HeadParams":
        """From a module with SB3's attribute names (`mlp_extractor.policy_net / value_net`, `action_net`, `value_net`, `log_std`): an
        `ActorCriticHead`, or an SB3 `ActorCriticPolicy`, whose configuration is checked against what the kernels compute."""
        _reject_policy_flags(policy)
        if not isinstance(getattr(policy, "log_std", None), torch.Tensor):
            raise ValueError("the policy has no log_std: the HIP policy head computes the diagonal Gaussian of a continuous (Box) action space only")
        return HeadParams(H.linear_pairs(policy.mlp_extractor.policy_net, "mlp_extractor.policy_net", nn.Tanh, "policy"),
                          H.linear_pairs(policy.mlp_extractor.value_net, "mlp_extractor.value_net", nn.Tanh, "policy"),
                          (policy.action_net.weight, policy.action_net.bias), (policy.value_net.weight, policy.value_net.bias), policy.log_std)


def _reject_policy_flags(policy):
    if getattr(policy, "use_sde", False):
        raise ValueError("use_sde=True (generalised state-dependent exploration) is not computed by the HIP policy head")
    if getattr(policy, "squash_output", False):
        raise ValueError("squash_output=True is not computed by the HIP policy head")
    if not getattr(policy, "share_features_extractor", True):
        raise ValueError("share_features_extractor=False: the HIP policy head takes one feature vector for both branches")


def _arch(x, params: HeadParams):
    """(F, A, pi widths, vf widths) with every shape checked; raises ValueError for a head outside the kernels' limits."""
    F = int(x.shape[-1])
    A = int(params.log_std.numel())
    H.check_float32(params.flat(), "policy")
    widths = []
    for name, br, head_name, head, hn in (("pi", params.pi, "pi head", params.action, A), ("vf", params.vf, "vf head", params.value, 1)):
        k, ws = H.layer_widths(F, br, name, "policy", "branch")
        H.check_head_linear(head_name, head, hn, k)
        widths.append(ws)
    H.check_limits((F,) + widths[0] + widths[1], A)
    return F, A, widths[0], widths[1]


def _desc(arch, flat):
    """m3l_policy_desc over the tensors of `flat` (HeadParams.flat order); the caller keeps `flat` alive while the descriptor is in use."""
    F, A, pi, vf = arch
    d = L.PolicyDesc()
    d.features, d.actions, d.n_pi, d.n_vf = F, A, len(pi), len(vf)
    it = iter(flat)
    for l, w in enumerate(pi):
        d.pi_width[l] = w
        d.pi_weight[l], d.pi_bias[l] = next(it).data_ptr(), next(it).data_ptr()
    for l, w in enumerate(vf):
        d.vf_width[l] = w
        d.vf_weight[l], d.vf_bias[l] = next(it).data_ptr(), next(it).data_ptr()
    d.action_weight, d.action_bias = next(it).data_ptr(), next(it).data_ptr()
    d.value_weight, d.value_bias = next(it).data_ptr(), next(it).data_ptr()
    d.log_std = next(it).data_ptr()
    return d


class ActorCriticEvalFn(torch.autograd.Function):
    """(features (B, F), actions (B, A), arch, store, *parameters in HeadParams.flat order) -> values (B,), log_prob (B,), entropy (B,).  One
    launch; the backward (2 launches) returns d features and every parameter gradient.  Actions take no gradient.  `store`: a backward may
    follow, so the forward gets a workspace and leaves its activations there.  The caller decides it (`evaluate_actions`): inside `forward` the
    grad mode is always off and `ctx.needs_input_grad` is each input's own `requires_grad` whatever the mode, so neither can tell."""

    @staticmethod
    def forward(ctx, x, actions, arch, store, *params):
        B = x.shape[0]
        flat = [_dev(t) for t in params]
        lib = L.lib()
        d = _desc(arch, flat)
        e = lambda: torch.empty(B, dtype=torch.float32, device=x.device)      # noqa: E731
        values, logp, entropy = e(), e(), e()
        ws = _ws(lib.m3l_policy_ws_bytes(C.byref(d), B), x.device) if store else None
        L.check(lib.m3l_policy_eval_fwd(C.byref(d), B, L.ptr(x), L.ptr(actions), L.ptr(ws), L.ptr(values), L.ptr(logp), L.ptr(entropy), _stream()),
                "m3l_policy_eval_fwd")
        ctx.saved = (x, actions, arch, flat, ws)
        ctx.set_materialize_grads(False)
        return values, logp, entropy

    @staticmethod
    def backward(ctx, dvalues, dlogp, dentropy):
        x, actions, arch, flat, ws = ctx.saved
        if ws is None:
            raise H.no_workspace("ActorCriticEvalFn")
        B = x.shape[0]
        dv, dl, de = (None if g is None else _dev(g).reshape(B) for g in (dvalues, dlogp, dentropy))
        grads = [torch.empty_like(t) for t in flat]
        dx = torch.empty_like(x)
        d, gd = _desc(arch, flat), _desc(arch, grads)
        L.check(L.lib().m3l_policy_eval_bwd(C.byref(d), B, L.ptr(x), L.ptr(actions), L.ptr(dv), L.ptr(dl), L.ptr(de), L.ptr(ws), L.ptr(dx), C.byref(gd),
                                            _stream()), "m3l_policy_eval_bwd")
        return (dx, None, None, None) + tuple(grads)


class PPOLossFn(torch.autograd.Function):
    """(log_prob, values, entropy, old_log_prob, advantages, returns, old_values or None, clip_range, clip_range_vf or None, ent_coef, vf_coef,
    normalize_advantage) -> loss 0-d, stats (5,) in STAT_NAMES order (no gradient).  One launch each way; the gradient goes to log_prob, values
    and entropy."""

    @staticmethod
    def forward(ctx, logp, values, entropy, old_logp, adv, returns, old_values, clip_range, clip_range_vf, ent_coef, vf_coef, normalize):
        B = logp.numel()
        dev = logp.device
        loss = torch.empty((), dtype=torch.float32, device=dev)
        stats = torch.empty(5, dtype=torch.float32, device=dev)
        c_logp = torch.empty(B, dtype=torch.float32, device=dev)
        c_v = torch.empty(B, dtype=torch.float32, device=dev)
        L.check(L.lib().m3l_policy_ppo_loss_fwd(L.ptr(logp), L.ptr(values), L.ptr(entropy), L.ptr(old_logp), L.ptr(adv), L.ptr(returns), L.ptr(old_values), B,
                                                float(clip_range), -1.0 if clip_range_vf is None else float(clip_range_vf), float(ent_coef), float(vf_coef),
                                                int(bool(normalize)), L.ptr(loss), L.ptr(stats), L.ptr(c_logp), L.ptr(c_v), _stream()),
                "m3l_policy_ppo_loss_fwd")
        ctx.saved = (c_logp, c_v, B, float(ent_coef))
        ctx.mark_non_differentiable(stats)
        return loss, stats

    @staticmethod
    def backward(ctx, dloss, _dstats):
        c_logp, c_v, B, ent_coef = ctx.saved
        e = lambda: torch.empty(B, dtype=torch.float32, device=c_logp.device)      # noqa: E731
        dlogp, dvalues, dentropy = e(), e(), e()
        L.check(L.lib().m3l_policy_ppo_loss_bwd(L.ptr(_dev(dloss)), L.ptr(c_logp), L.ptr(c_v), B, ent_coef, L.ptr(dlogp), L.ptr(dvalues), L.ptr(dentropy),
                                                _stream()), "m3l_policy_ppo_loss_bwd")
        return (dlogp, dvalues, dentropy) + (None,) * 9


class PPOStats(torch.Tensor):
    """The five statistics of a loss call as a device tensor, in STAT_NAMES order."""

    def stats_dict(self):
        """{name: float}: ONE device-to-host copy for all five (the reference makes five, `ppo_mae.py:297, 298, 312, 321, 331`)."""
        return dict(zip(STAT_NAMES, self.detach().as_subclass(torch.Tensor).cpu().tolist()))


def evaluate_actions(params: HeadParams, features, actions):
    """values (B,), log_prob (B,), entropy (B,) of `actions` (B, A) under the head `params` at `features` (B, F); differentiable in the features
    and every parameter.  Under `no_grad`, or when nothing requires a gradient, no workspace is allocated and no activation is stored."""
    H.require_params(params.flat(), "policy head parameter")
    x = H.features_of(features, on_tape=True)          # the features take a gradient
    arch = _arch(x, params)
    a = _rows(actions.reshape(actions.shape[0], -1) if actions.dim() != 2 else actions, "actions", arch[1])
    if a.shape[0] != x.shape[0]:
        raise ValueError(f"{x.shape[0]} feature rows but {a.shape[0]} action rows")
    flat = params.flat()
    store = torch.is_grad_enabled() and (x.requires_grad or any(t.requires_grad for t in flat))      # under no_grad nothing is stored
    return ActorCriticEvalFn.apply(x, a, arch, store, *flat)


@torch.no_grad()
def act(params: HeadParams, features, deterministic=False, noise=None):
    """actions (B, A) = mu + exp(log_std) * noise (mu when deterministic), values (B,), log_prob (B,) of those actions.  One launch, nothing kept
    for a backward.  `noise` (B, A): the standard-normal draw; made with torch.randn when not given."""
    H.require_params(params.flat(), "policy head parameter")
    x = H.features_of(features, on_tape=False)
    arch = _arch(x, params)
    B, A = x.shape[0], arch[1]
    noise = H.noise_of(noise, B, A, x.device, deterministic)
    flat = [_dev(t) for t in params.flat()]
    d = _desc(arch, flat)
    actions = torch.empty(B, A, dtype=torch.float32, device=x.device)
    values = torch.empty(B, dtype=torch.float32, device=x.device)
    logp = torch.empty(B, dtype=torch.float32, device=x.device)
    L.check(L.lib().m3l_policy_act(C.byref(d), B, L.ptr(x), L.ptr(noise), L.ptr(actions), L.ptr(values), L.ptr(logp), _stream()), "m3l_policy_act")
    return actions, values, logp


def ppo_loss_from(values, log_prob, entropy, old_log_prob, advantages, returns, clip_range, ent_coef=0.0, vf_coef=0.5, clip_range_vf=None, old_values=None,
                  normalize_advantage=True):
    """The PPO loss of `ppo_mae.py:281-331` from the outputs of `evaluate_actions` -> (loss 0-d, stats PPOStats (5,))."""
    B = log_prob.numel()
    for t, what in ((values, "values"), (log_prob, "log_prob"), (entropy, "entropy")):
        _require_cuda(t, what)
        if t.dtype != torch.float32 or t.numel() != B:
            raise ValueError(f"{what}: {B} float32 values expected, got {tuple(t.shape)} {t.dtype}")
    if clip_range_vf is not None and old_values is None:
        raise ValueError("clip_range_vf needs old_values")
    if clip_range_vf is not None and not clip_range_vf > 0:
        raise ValueError("clip_range_vf must be positive; pass None for no value clipping")
    ov = _vec(old_values, "old_values", B) if clip_range_vf is not None else None
    loss, stats = PPOLossFn.apply(log_prob.contiguous().reshape(B), values.contiguous().reshape(B), entropy.contiguous().reshape(B),
                                  _vec(old_log_prob, "old_log_prob", B), _vec(advantages, "advantages", B), _vec(returns, "returns", B), ov,
                                  clip_range, clip_range_vf, ent_coef, vf_coef, normalize_advantage)
    return loss, stats.as_subclass(PPOStats)


def ppo_loss(params: HeadParams, features, actions, old_log_prob, advantages, returns, clip_range, ent_coef=0.0, vf_coef=0.5, clip_range_vf=None,
             old_values=None, normalize_advantage=True):
    """evaluate_actions + the PPO loss: 2 launches forward, 3 backward -> (loss, stats)."""
    values, log_prob, entropy = evaluate_actions(params, features, actions)
    return ppo_loss_from(values, log_prob, entropy, old_log_prob, advantages, returns, clip_range, ent_coef, vf_coef, clip_range_vf, old_values,
                         normalize_advantage)


class _MlpExtractor(nn.Module):
    """`policy_net` and `value_net` as nn.Sequential of Linear at the even and Tanh at the odd indices (SB3's MlpExtractor names)."""

    def __init__(self, features_dim, pi, vf):
        super().__init__()
        self.policy_net = H.mlp(features_dim, pi, nn.Tanh)
        self.value_net = H.mlp(features_dim, vf, nn.Tanh)
        self.latent_dim_pi = pi[-1] if pi else features_dim
        self.latent_dim_vf = vf[-1] if vf else features_dim


class ActorCriticHead(nn.Module):
    """The parameters of SB3's `ActorCriticPolicy` behind the features extractor, with its names and layouts (`mlp_extractor.policy_net.{0,2,..}`,
    `mlp_extractor.value_net.{0,2,..}`, `action_net`, `value_net`, `log_std`; created in the order of SB3 2.x's `_build`), so an SB3 policy's state
    dict loads with strict=True, and the methods of that policy computed by the HIP kernels.  Initial values follow SB3's `ortho_init` (orthogonal
    weights with gain sqrt 2 / 0.01 / 1, zero biases); parity with SB3 is unpinned (SB3 is not part of the reference tree)."""

    def __init__(self, features_dim, action_dim, net_arch=None, log_std_init=0.0, activation_fn=nn.Tanh, ortho_init=True, use_sde=False,
                 squash_output=False, share_features_extractor=True):
        super().__init__()
        if activation_fn is not nn.Tanh:
            raise ValueError(f"activation_fn={getattr(activation_fn, '__name__', activation_fn)}: the HIP policy head computes Tanh only")
        self.use_sde, self.squash_output, self.share_features_extractor = bool(use_sde), bool(squash_output), bool(share_features_extractor)
        _reject_policy_flags(self)
        self.features_dim, self.action_dim, pi, vf = H.head_dims(features_dim, action_dim, net_arch, [64, 64], "vf", "policy", "branch", "features_dim")
        action_dim = self.action_dim
        self.mlp_extractor = _MlpExtractor(self.features_dim, pi, vf)
        self.action_net = nn.Linear(self.mlp_extractor.latent_dim_pi, action_dim)
        self.log_std = nn.Parameter(torch.ones(action_dim) * float(log_std_init))
        self.value_net = nn.Linear(self.mlp_extractor.latent_dim_vf, 1)
        if ortho_init:
            for module, gain in ((self.mlp_extractor, 2 ** 0.5), (self.action_net, 0.01), (self.value_net, 1.0)):
                for m in module.modules():
                    if isinstance(m, nn.Linear):
                        nn.init.orthogonal_(m.weight, gain=gain)
                        m.bias.data.fill_(0.0)

    def params(self) -> HeadParams:
        return HeadParams.from_policy(self)

    def forward(self, features, deterministic=False, noise=None):
        """(actions, values, log_prob) as `ActorCriticPolicy.forward` after `extract_features`; no gradient (rollouts run under no_grad)."""
        return act(self.params(), features, deterministic, noise)

    def evaluate_actions(self, features, actions):
        """(values, log_prob, entropy); values are flat (B,), as `ppo_mae.py:281` makes them."""
        return evaluate_actions(self.params(), features, actions)

    def predict_values(self, features):
        return act(self.params(), features, deterministic=True)[1]

    def ppo_loss(self, features, actions, old_log_prob, advantages, returns, clip_range, ent_coef=0.0, vf_coef=0.5, clip_range_vf=None, old_values=None,
                 normalize_advantage=True):
        return ppo_loss(self.params(), features, actions, old_log_prob, advantages, returns, clip_range, ent_coef, vf_coef, clip_range_vf, old_values,
                        normalize_advantage)
