#!/usr/bin/env python3
"""Golden results of the PPO loss lines, recorded from the reference's own `PPO_MAE.train` (runs only where /root/reference is mounted).

`models/ppo_mae.py` is imported from where it lies with inert stubs for its non-arithmetic imports (gymnasium, stable_baselines3.*,
utils.pretrain_utils), as make_golden.py does, and `PPO_MAE.train` (ppo_mae.py:200-367) is called, unbound, on a duck-typed `self`:

  rollout_buffer   yields ONE minibatch (the whole batch) whose observations are {"image": features (B, F)}
  policy           written here from torch primitives (nn.Linear, nn.Tanh, torch.distributions.Normal): SB3's ActorCriticPolicy head behind the
                   extractor, parameters under SB3's names; `evaluate_actions` records what it returns; its optimizer does nothing
  n_epochs = 1, max_grad_norm = 1e9 (clip_grad_norm_ multiplies by exactly 1), mae = a zero loss, separate_optimizer = False, target_kl = None
  logger           records every `record` call
  clip_range / clip_range_vf   constant schedules

Everything runs in float64.  `train` could be driven this way, so the restatement of tests/ppo_cases.py is pinned to the reference's own lines:
per case the file holds the inputs, `values` / `log_prob` / `entropy` as the policy returned them, the logged losses and statistics, and the gradient
`loss.backward()` left in every parameter and in the features.  The policy's arithmetic is this file's (SB3 is not in the reference tree:
parity unpinned), the loss arithmetic is the reference's.

Cases (B = 24, F = 32, widths 32 / 32, A = 3): default flags, clip_range_vf set, normalize_advantage = False, B = 1.  The file is about 270 KB:
the 4.5 k parameters of a case in float32 and their gradients in float64 are most of it.

Usage:  python tests/golden/make_golden_ppo_head.py        (rewrites tests/golden/ppo_head_step.npz)
"""
import importlib.util
import os
import sys
import types

import numpy as np
import torch
from torch import nn

HERE = os.path.dirname(os.path.abspath(__file__))
REF = "/root/reference"
sys.path.insert(0, os.path.dirname(HERE))
import ppo_cases as PC  # noqa: E402


def _install_stubs():
    def mod(name, **attrs):
        m = types.ModuleType(name)
        m.__dict__.update(attrs)
        sys.modules[name] = m
        return m

    class _Dummy:
        def __init__(self, *a, **k):
            pass

    kinds = {n: type(n, (_Dummy,), {}) for n in ("Box", "Discrete", "MultiDiscrete", "MultiBinary", "Space", "Dict")}
    gym = mod("gymnasium", **kinds)
    gym.spaces = mod("gymnasium.spaces", **kinds)
    sb3 = mod("stable_baselines3")
    sb3.common = mod("stable_baselines3.common")
    mod("stable_baselines3.common.on_policy_algorithm", OnPolicyAlgorithm=_Dummy)
    mod("stable_baselines3.common.policies", ActorCriticCnnPolicy=_Dummy, ActorCriticPolicy=_Dummy, BasePolicy=_Dummy, MultiInputActorCriticPolicy=_Dummy)
    mod("stable_baselines3.common.type_aliases", GymEnv=object, MaybeCallback=object, Schedule=object)
    mod("stable_baselines3.common.utils", explained_variance=lambda y_pred, y_true: float("nan"), get_schedule_fn=lambda v: (lambda _progress: v))
    utils = mod("utils")
    utils.pretrain_utils = mod("utils.pretrain_utils", vt_load=lambda obs, frame_stack=1: obs)
    return gym.spaces


def _load_reference():
    spaces = _install_stubs()
    spec = importlib.util.spec_from_file_location("ref_ppo_mae", os.path.join(REF, "models", "ppo_mae.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m, spaces


class Policy(nn.Module):
    """SB3's ActorCriticPolicy behind its features extractor (net_arch = dict(pi, vf), Tanh, DiagGaussianDistribution), from torch primitives."""

    def __init__(self, arch, P):
        super().__init__()
        Fd, pi, vf, A = arch

        def seq(widths):
            mods, k = [], Fd
            for w in widths:
                mods += [nn.Linear(k, w), nn.Tanh()]
                k = w
            return nn.Sequential(*mods), k
        self.mlp_extractor = nn.Module()
        self.mlp_extractor.policy_net, kp = seq(pi)
        self.mlp_extractor.value_net, kv = seq(vf)
        self.action_net = nn.Linear(kp, A)
        self.log_std = nn.Parameter(torch.zeros(A))
        self.value_net = nn.Linear(kv, 1)
        self.double()
        self.load_state_dict({k: torch.from_numpy(v).double() for k, v in P.items()}, strict=True)
        self.optimizer = types.SimpleNamespace(zero_grad=lambda: None, step=lambda: None)
        self.seen = {}

    def set_training_mode(self, mode):
        self.train(mode)

    def evaluate_actions(self, obs, actions):
        x = obs["image"]
        mean = self.action_net(self.mlp_extractor.policy_net(x))
        dist = torch.distributions.Normal(mean, torch.ones_like(mean) * self.log_std.exp())
        values = self.value_net(self.mlp_extractor.value_net(x))
        out = values, dist.log_prob(actions).sum(dim=1), dist.entropy().sum(dim=1)
        self.seen = dict(values=out[0].detach().flatten().numpy().copy(), log_prob=out[1].detach().numpy().copy(), entropy=out[2].detach().numpy().copy())
        return out


class Logger:
    def __init__(self):
        self.rec = {}

    def record(self, key, value, exclude=None):
        self.rec[key] = value


def run_case(ref, spaces, c):
    t = lambda k: torch.from_numpy(c[k]).double()      # noqa: E731
    x = t("x").requires_grad_(True)
    policy = Policy(c["arch"], c["params"])
    batch = types.SimpleNamespace(observations={"image": x}, actions=t("actions"), advantages=t("advantages"), old_log_prob=t("old_log_prob"),
                                  old_values=t("old_values"), returns=t("returns"))
    B = x.shape[0]
    me = types.SimpleNamespace(
        policy=policy, _update_learning_rate=lambda opt: None, clip_range=lambda _p: c["clip_range"],
        clip_range_vf=None if c["clip_range_vf"] is None else (lambda _p: c["clip_range_vf"]), _current_progress_remaining=1.0, n_epochs=1,
        rollout_buffer=types.SimpleNamespace(get=lambda batch_size: iter([batch]), values=np.zeros(B), returns=np.zeros(B)), batch_size=B,
        mae_batch_size=B, separate_optimizer=False, mae=lambda obs: torch.zeros((), dtype=torch.float64, requires_grad=True),
        mae_optimizer=None, action_space=spaces.Box(), use_sde=False, normalize_advantage=c["normalize_advantage"], ent_coef=c["ent_coef"],
        vf_coef=c["vf_coef"], target_kl=None, verbose=0, max_grad_norm=1e9, _n_updates=0, logger=Logger())
    ref.PPO_MAE.train(me)
    rec = me.logger.rec
    out = {"values": policy.seen["values"], "log_prob": policy.seen["log_prob"], "entropy": policy.seen["entropy"], "loss": np.float64(rec["train/loss"]),
           "policy_loss": np.float64(rec["train/policy_gradient_loss"]), "value_loss": np.float64(rec["train/value_loss"]),
           "entropy_loss": np.float64(rec["train/entropy_loss"]), "clip_fraction": np.float64(rec["train/clip_fraction"]),
           "approx_kl": np.float64(rec["train/approx_kl"]), "grad/x": x.grad.numpy()}
    for k, p in policy.named_parameters():
        out["grad/" + k] = p.grad.numpy()
    assert me._n_updates == 1 and rec["train/clip_range"] == c["clip_range"]
    return out


GOLDEN_CASES = {"default": (24, "default"), "vfclip": (24, "vfclip"), "nonorm": (24, "nonorm"), "b1": (1, "default")}


def main():
    ref, spaces = _load_reference()
    z = {}
    for i, (name, (B, flags)) in enumerate(GOLDEN_CASES.items()):
        c = PC.make_inputs(PC.ARCHS["golden"], B, flags, late=B > 1, seed=500 + i)
        for k in ("x", "actions", "old_log_prob", "advantages", "returns", "old_values"):
            z[f"{name}/in/{k}"] = c[k]
        for k, v in c["params"].items():
            z[f"{name}/param/{k}"] = v
        z[f"{name}/flags"] = np.array([c["clip_range"], -1.0 if c["clip_range_vf"] is None else c["clip_range_vf"], float(c["normalize_advantage"]),
                                       c["ent_coef"], c["vf_coef"]], dtype=np.float64)
        for k, v in run_case(ref, spaces, c).items():
            z[f"{name}/out/{k}"] = v
        print(name, {k: float(z[f"{name}/out/{k}"]) for k in ("loss",) + PC.STAT_NAMES})
    path = os.path.join(HERE, "ppo_head_step.npz")
    np.savez_compressed(path, **z)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
