#!/usr/bin/env python3
"""Golden results of the head's part of a SAC gradient step, recorded from the reference's own `SAC_MAE.train` (runs only where /root/reference
is mounted).

`models/sac_mae.py` is imported from where it lies with inert stubs for its non-arithmetic imports (gymnasium, stable_baselines3.*,
models.sac_mae_policy, utils.pretrain_utils), as make_golden_ppo_head.py does, and `SAC_MAE.train` (sac_mae.py:223-382) is called, unbound, on a
duck-typed `self`:

  gradient_steps = 1, replay_buffer.sample   returns ONE batch whose observations / next_observations are {"image": features (B, F)}
  actor, critic, critic_target   written here from torch primitives (tests/sac_cases.py's functions over real nn.Linear parameters under SB3's
                   names), float64; the actor consumes recorded noise in call order; the critics detach their features, as a shared extractor
                   makes SB3's do; each records what it returns
  optimizers       zero_grad really zeroes, step records the gradients present at that moment and changes nothing; ent_coef_optimizer the same
                   over a real log_ent_coef (the fixed case has ent_coef_tensor and no optimizer)
  mae = a zero loss, separate_optimizer = False, target_update_interval = 1, empty batch_norm_stats, a recording logger
  polyak_update    is SB3's, so it is restated in the stub (target.mul_(1 - tau); target.add_(param, alpha=tau))

Everything runs in float64.  `train` could be driven this way from its first line to its last, so the step of tests/sac_cases.py is pinned to the
reference's own lines; the actor's and the critics' arithmetic is sac_cases' (SB3 is not in the reference tree: parity unpinned).  Per case the
file holds the inputs and noise, `a_pi`, `log_prob` and `target_q` as the stubs saw them, the four logged values, every recorded gradient (the
critic's after the critic loss, the actor's and x's after the actor loss, log_ent_coef's) and the target critics after the Polyak update.

Cases (F = 32, widths 32 / 32, A = 3): auto entropy coefficient, a fixed one, clamped log_std entries, each at B = 24, and B = 1.  About 570 KB:
a case holds 11 k float32 parameters, 6.7 k float64 gradients and 4.4 k float64 target values, which do not compress.

Usage:  python tests/golden/make_golden_sac_head.py        (rewrites tests/golden/sac_head_step.npz)
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
import sac_cases as SC  # noqa: E402


def _polyak_update(params, target_params, tau):
    """SB3's stable_baselines3.common.utils.polyak_update."""
    with torch.no_grad():
        for param, target_param in zip(list(params), list(target_params)):
            target_param.data.mul_(1 - tau)
            torch.add(target_param.data, param.data, alpha=tau, out=target_param.data)


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
    mod("stable_baselines3.common.buffers", ReplayBuffer=_Dummy)
    mod("stable_baselines3.common.noise", ActionNoise=_Dummy)
    mod("stable_baselines3.common.off_policy_algorithm", OffPolicyAlgorithm=_Dummy)
    mod("stable_baselines3.common.policies", BasePolicy=_Dummy, ContinuousCritic=_Dummy)
    mod("stable_baselines3.common.type_aliases", GymEnv=object, MaybeCallback=object, Schedule=object)
    mod("stable_baselines3.common.utils", get_parameters_by_name=lambda model, names: [], polyak_update=_polyak_update)
    mod("stable_baselines3.sac")
    mod("stable_baselines3.sac.policies", Actor=_Dummy, CnnPolicy=_Dummy, MlpPolicy=_Dummy, MultiInputPolicy=_Dummy, SACPolicy=_Dummy)
    models = mod("models")
    models.sac_mae_policy = mod("models.sac_mae_policy", MAESACPolicy=_Dummy)
    utils = mod("utils")
    utils.pretrain_utils = mod("utils.pretrain_utils", vt_load=lambda obs, frame_stack=1: obs)


def _load_reference():
    _install_stubs()
    spec = importlib.util.spec_from_file_location("ref_sac_mae", os.path.join(REF, "models", "sac_mae.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


class RecordingOptimizer:
    """zero_grad really zeroes; step records the gradients present at that moment and changes nothing."""

    def __init__(self, named):
        self.named, self.steps = dict(named), []

    def zero_grad(self):
        for p in self.named.values():
            p.grad = None

    def step(self):
        self.steps.append({k: p.grad.detach().numpy().copy() for k, p in self.named.items()})


def _mlp(k, widths, out=None):
    mods = []
    for w in widths:
        mods += [nn.Linear(k, w), nn.ReLU()]
        k = w
    if out is not None:
        mods.append(nn.Linear(k, out))
    return nn.Sequential(*mods), k


class Actor(nn.Module):
    """SB3's Actor behind the extractor (use_sde = False), from torch primitives; consumes the recorded noise in call order."""

    def __init__(self, arch, P, noises):
        super().__init__()
        Fd, pi, _, A = arch
        self.latent_pi, k = _mlp(Fd, pi)
        self.mu, self.log_std = nn.Linear(k, A), nn.Linear(k, A)
        self.double()
        self.load_state_dict({k[len("actor."):]: torch.from_numpy(v).double() for k, v in P.items() if k.startswith("actor.")}, strict=True)
        self.optimizer = RecordingOptimizer(("actor." + k, p) for k, p in self.named_parameters())
        self.noises, self.seen = list(noises), []

    def action_log_prob(self, obs):
        o = SC.actor_forward({"actor." + k: p for k, p in self.named_parameters()}, obs["image"], self.noises.pop(0))
        self.seen.append((o["actions"].detach().numpy().copy(), o["log_prob"].detach().numpy().copy()))
        return o["actions"], o["log_prob"]


class Critic(nn.Module):
    """SB3's ContinuousCritic with n_critics = 2 and a shared extractor (the features enter detached), from torch primitives."""

    def __init__(self, arch, P, prefix):
        super().__init__()
        Fd, _, qf, A = arch
        self.prefix = prefix
        self.qf0, _ = _mlp(Fd + A, qf, 1)
        self.qf1, _ = _mlp(Fd + A, qf, 1)
        self.double()
        self.load_state_dict({k[len(prefix) + 1:]: torch.from_numpy(v).double() for k, v in P.items() if k.startswith(prefix + ".")}, strict=True)
        self.optimizer = RecordingOptimizer((prefix + "." + k, p) for k, p in self.named_parameters())

    def forward(self, obs, actions):
        q, _ = SC.critic_forward({self.prefix + "." + k: p for k, p in self.named_parameters()}, self.prefix, obs["image"], actions)
        return tuple(qc.reshape(-1, 1) for qc in q)


class Logger:
    def __init__(self):
        self.rec = {}

    def record(self, key, value, exclude=None):
        self.rec[key] = value


def run_case(ref, c):
    t = lambda k: torch.from_numpy(c[k]).double()      # noqa: E731
    x = t("x").requires_grad_(True)
    arch, P = c["arch"], c["params"]
    actor = Actor(arch, P, [t("noise_pi"), t("noise_next")])
    critic, target = Critic(arch, P, "critic"), Critic(arch, P, "critic_target").requires_grad_(False)
    seen_target = {}

    def sample(batch_size, env=None):
        return types.SimpleNamespace(observations={"image": x}, next_observations={"image": t("x_next")}, actions=t("a_replay"),
                                     rewards=t("rewards").reshape(-1, 1), dones=t("dones").reshape(-1, 1))
    real_mse = ref.F.mse_loss

    def mse(q, target_q, *a, **k):          # target_q as the reference formed it
        seen_target["target_q"] = target_q.detach().numpy().copy().ravel()
        return real_mse(q, target_q, *a, **k)
    ref.F = types.SimpleNamespace(mse_loss=mse)
    B = x.shape[0]
    me = types.SimpleNamespace(
        policy=types.SimpleNamespace(set_training_mode=lambda mode: None, optimizer=types.SimpleNamespace(zero_grad=lambda: None)),
        actor=actor, critic=critic, critic_target=target, _update_learning_rate=lambda opts: None, replay_buffer=types.SimpleNamespace(sample=sample),
        _vec_normalize_env=None, mae_batch_size=B, separate_optimizer=False, mae=lambda obs: torch.zeros((), dtype=torch.float64, requires_grad=True),
        mae_optimizer=None, use_sde=False, gamma=c["gamma"], tau=c["tau"], target_update_interval=1, batch_norm_stats=[], batch_norm_stats_target=[],
        target_entropy=c["target_entropy"], _n_updates=0, logger=Logger())
    if c["auto"]:
        me.log_ent_coef = torch.tensor([c["log_ent_coef"]], dtype=torch.float64, requires_grad=True)
        me.ent_coef_optimizer = RecordingOptimizer([("log_ent_coef", me.log_ent_coef)])
    else:
        me.log_ent_coef, me.ent_coef_optimizer = None, None
        me.ent_coef_tensor = torch.tensor(c["ent_coef"], dtype=torch.float64)
    try:
        ref.SAC_MAE.train(me, 1, batch_size=B)
    finally:
        ref.F = types.SimpleNamespace(mse_loss=real_mse)
    rec = me.logger.rec
    assert me._n_updates == 1 and len(actor.seen) == 2 and not actor.noises and len(critic.optimizer.steps) == 1 and len(actor.optimizer.steps) == 1
    out = {"a_pi": actor.seen[0][0], "log_prob": actor.seen[0][1], "target_q": seen_target["target_q"], "ent_coef": np.float64(rec["train/ent_coef"]),
           "actor_loss": np.float64(rec["train/actor_loss"]), "critic_loss": np.float64(rec["train/critic_loss"]), "grad/x": x.grad.numpy()}
    if c["auto"]:
        out["ent_coef_loss"] = np.float64(rec["train/ent_coef_loss"])
        out["grad/log_ent_coef"] = me.ent_coef_optimizer.steps[0]["log_ent_coef"]
    for k, v in list(critic.optimizer.steps[0].items()) + list(actor.optimizer.steps[0].items()):
        out["grad/" + k] = v
    for k, p in target.named_parameters():
        out["target/critic_target." + k] = p.detach().numpy().copy()
    return out


# name -> (B, hi, auto)
GOLDEN_CASES = {"auto": (24, False, True), "fixed": (24, False, False), "clamped": (24, True, True), "b1": (1, False, True)}
INPUTS = ("x", "x_next", "noise_pi", "noise_next", "a_replay", "rewards", "dones")


def golden_inputs(name):
    B, hi, auto = GOLDEN_CASES[name]
    return SC.make_inputs(SC.ARCHS["golden"], B, hi, auto, seed=700 + list(GOLDEN_CASES).index(name))


def main():
    ref = _load_reference()
    z = {}
    for name in GOLDEN_CASES:
        c = golden_inputs(name)
        for k in INPUTS:
            z[f"{name}/in/{k}"] = c[k]
        for k, v in c["params"].items():
            z[f"{name}/param/{k}"] = v
        z[f"{name}/flags"] = np.array([c["gamma"], c["tau"], float(c["auto"]), c["log_ent_coef"], c["ent_coef"], c["target_entropy"], float(c["hi"])],
                                      dtype=np.float64)
        for k, v in run_case(ref, c).items():
            z[f"{name}/out/{k}"] = v
        print(name, {k: float(z[f"{name}/out/{k}"]) for k in ("actor_loss", "critic_loss", "ent_coef")})
    path = os.path.join(HERE, "sac_head_step.npz")
    np.savez_compressed(path, **z)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
