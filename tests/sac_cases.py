"""Float64 restatement of the SAC policy head and of the head's part of one gradient step, and the inputs of its tests (test_sac_head_cpu.py,
test_sac_head_gpu.py, golden/make_golden_sac_head.py, tools/sac_head_bench.py).

The head — Stable-Baselines3's SACPolicy behind its features extractor as MAESACPolicy configures it (nn.ReLU, n_critics = 2,
share_features_extractor = True, use_sde = False) — is built from torch primitives (nn.functional.linear, torch.relu, torch.clamp, torch.tanh,
torch.distributions.Normal, autograd).  SB3 is not part of the reference tree, so that part restates SB3 2.x's Actor.action_log_prob,
SquashedDiagGaussianDistribution and ContinuousCritic: PARITY UNPINNED.  The step follows models/sac_mae.py:303-366 line by line, and
test_sac_head_cpu.py pins it to results recorded from the reference's own `SAC_MAE.train` (golden/sac_head_step.npz).

Inputs are trained-like, not initialisation statistics: every hidden layer's weights are scaled until its pre-activations have a standard
deviation of 1.6 (a fifth of the units beyond |pre| = 2), mu has a standard deviation of 1.3 so that |u| reaches 3 to 4, the pre-clamp log_std
is centred on -1 and, in the `hi` cases, on 1.7 so that more than 5 % of its entries lie above the clamp's upper edge.

What the float32 / float64 comparisons rest on is made true of the inputs by `settle`, which nudges biases until, in float64, over every
evaluation the tests make (the actor at x and x', both critics at (x, a_replay) and (x, a_pi), both target critics at (x', a')):
  * every ReLU pre-activation has |pre| >= GATE_MARGIN;
  * |q0 - q1| >= TIE_MARGIN on every row of the target pair and of the (x, a_pi) pair;
  * no pre-clamp log_std lies within CLAMP_MARGIN of -20 or 2.
GATE_MARGIN: the largest |pre_f32 - pre_f64| of the restatement over all GPU and golden cases, measured on the CPU, is 4.8e-6 (a256_b130),
MEASURED_PRE_ERR rounds it up to 5e-6; the margin is 2e-4, 40 times that.  test_sac_head_cpu.py measures the figure again and asserts that it
stays under MEASURED_PRE_ERR and that the margin is at least 8 times it."""
import math
from functools import lru_cache

import numpy as np
import torch
from torch.nn import functional as F

PRE_STD = 1.6
MEASURED_PRE_ERR = 5e-6
GATE_MARGIN = 2e-4
TIE_MARGIN = 1e-3
CLAMP_MARGIN = 1e-3
LOG_STD_MIN, LOG_STD_MAX = -20.0, 2.0
EPS = 1e-6
GAMMA, TAU = 0.99, 0.005

# (features, pi widths, qf widths, actions)
ARCHS = {
    "a64": (64, (64, 64), (64, 64), 3),            # F + A = 67: residue 3
    "a256": (256, (256, 256), (256, 256), 7),      # the workload's own widths, F + A = 263
    "mixed": (32, (32,), (64, 48, 16), 1),         # residue 1
    "nohid": (48, (), (16,), 2),                   # residue 2
    "aligned": (16, (16,), (16,), 16),             # residue 0
    "amax": (16, (32,), (), 64),                   # widest A, no hidden critic layer
    "golden": (32, (32, 32), (32, 32), 3),
}

# name -> (arch, B, hi: log_std entries above the clamp, auto: ent_coef = exp(log_ent_coef) with its loss, else a fixed ent_coef)
GPU_CASES = {
    "a64_b1": ("a64", 1, False, True),
    "a64_b2": ("a64", 2, False, False),
    "a64_b3": ("a64", 3, False, True),
    "a64_b15": ("a64", 15, False, True),
    "a64_b17": ("a64", 17, True, True),
    "a64_b33": ("a64", 33, False, True),
    "a64_b63": ("a64", 63, False, False),
    "a64_b65": ("a64", 65, False, True),
    "a256_b130": ("a256", 130, True, True),
    "mixed_b15": ("mixed", 15, False, True),
    "mixed_b33": ("mixed", 33, True, False),
    "mixed_b65": ("mixed", 65, False, True),
    "nohid_b3": ("nohid", 3, False, True),
    "nohid_b33": ("nohid", 33, True, True),
    "aligned_b1": ("aligned", 1, False, False),
    "aligned_b33": ("aligned", 33, True, True),
    "amax_b3": ("amax", 3, False, True),
    "amax_b65": ("amax", 65, True, True),
}


def actor_names(arch):
    """State-dict names of the actor in SACHeadParams.actor_flat order."""
    names = []
    for l in range(len(arch[1])):
        names += [f"actor.latent_pi.{2 * l}.weight", f"actor.latent_pi.{2 * l}.bias"]
    return names + ["actor.mu.weight", "actor.mu.bias", "actor.log_std.weight", "actor.log_std.bias"]


def critic_names(arch, prefix="critic"):
    """State-dict names of the twin critics in SACHeadParams.critic_flat order."""
    names = []
    for c in range(2):
        for l in range(len(arch[2]) + 1):
            names += [f"{prefix}.qf{c}.{2 * l}.weight", f"{prefix}.qf{c}.{2 * l}.bias"]
    return names


def param_names(arch):
    """Every name of a SACHead's state dict, in creation order."""
    return actor_names(arch) + critic_names(arch) + critic_names(arch, "critic_target")


def stable_one_minus_tanh2(u):
    """1 - tanh(u)^2 as the kernels form it: 4 e / (1 + e)^2 with e = exp(-2 |u|)."""
    e = torch.exp(-2 * u.abs())
    return 4 * e / (1 + e) ** 2


def actor_forward(P, x, noise, stable=False):
    """SB3's Actor.action_log_prob after extract_features (SquashedDiagGaussianDistribution, rsample with the given standard-normal draw):
    actions, log_prob, and mu, the pre-clamp log_std, u and the ReLU pre-activations for the input checks.  stable: the log-probability in the
    kernels' form (the same function, without cancellation)."""
    h, pres, l = x, [], 0
    while f"actor.latent_pi.{2 * l}.weight" in P:
        pre = F.linear(h, P[f"actor.latent_pi.{2 * l}.weight"], P[f"actor.latent_pi.{2 * l}.bias"])
        pres.append(pre)
        h = torch.relu(pre)
        l += 1
    mu = F.linear(h, P["actor.mu.weight"], P["actor.mu.bias"])
    s_pre = F.linear(h, P["actor.log_std.weight"], P["actor.log_std.bias"])
    s = torch.clamp(s_pre, LOG_STD_MIN, LOG_STD_MAX)
    std = torch.exp(s)
    u = mu + std * noise
    a = torch.tanh(u)
    if stable:
        log_prob = (-0.5 * noise ** 2 - s - 0.5 * math.log(2 * math.pi)).sum(dim=1) - torch.log(stable_one_minus_tanh2(u) + EPS).sum(dim=1)
    else:
        log_prob = torch.distributions.Normal(mu, std).log_prob(u).sum(dim=1) - torch.log(1 - a ** 2 + EPS).sum(dim=1)
    return dict(actions=a, log_prob=log_prob, mu=mu, s_pre=s_pre, u=u, pre=pres)


def closed_form_log_prob(mu, s, u):
    """The header's formula."""
    a = torch.tanh(u)
    return (-(u - mu) ** 2 / (2 * torch.exp(s) ** 2) - s - 0.5 * math.log(2 * math.pi)).sum(-1) - torch.log(1 - a ** 2 + EPS).sum(-1)


def critic_forward(P, prefix, x, actions):
    """SB3's ContinuousCritic with a shared extractor: the features enter detached.  -> q (2, B), the ReLU pre-activations."""
    xa = torch.cat([x.detach(), actions], dim=1)
    qs, pres = [], []
    for c in range(2):
        h, l = xa, 0
        while f"{prefix}.qf{c}.{2 * l + 2}.weight" in P:
            pre = F.linear(h, P[f"{prefix}.qf{c}.{2 * l}.weight"], P[f"{prefix}.qf{c}.{2 * l}.bias"])
            pres.append(pre)
            h = torch.relu(pre)
            l += 1
        qs.append(F.linear(h, P[f"{prefix}.qf{c}.{2 * l}.weight"], P[f"{prefix}.qf{c}.{2 * l}.bias"]).flatten())
    return torch.stack(qs), pres


def as_torch(P, dtype=torch.float64, device="cpu"):
    """Leaves that take a gradient, except the target critics."""
    return {k: torch.from_numpy(np.asarray(v)).to(device=device, dtype=dtype).requires_grad_(not k.startswith("critic_target.")) for k, v in P.items()}


def step_ref(c, dtype=torch.float64, device="cpu", stable=False):
    """The head's part of one gradient step of SAC_MAE.train (models/sac_mae.py:303-366) in `dtype`, in the reference's order.  -> float64 numpy:
    a_pi, log_prob, ent_coef, ent_coef_loss (auto cases), target_q, q_replay, critic_loss, q_pi, actor_loss; grad: the critic's after the critic
    loss, the actor's and x's after the actor loss, log_ent_coef's; grad_critic_from_actor_loss: what the reference leaves in the critic after
    the actor loss (discarded at :347; the HIP head does not compute it); target: the target critics after the Polyak update; and the quantities
    of the input conditions."""
    P = as_torch(c["params"], dtype, device)
    t = lambda k: torch.from_numpy(c[k]).to(device=device, dtype=dtype)      # noqa: E731
    x = t("x").requires_grad_(True)
    n64 = lambda v: v.detach().double().cpu().numpy()      # noqa: E731
    out, grad = {}, {}
    act = actor_forward(P, x, t("noise_pi"), stable)                                                        # :303
    a_pi, log_prob = act["actions"], act["log_prob"].reshape(-1, 1)                                         # :304
    if c["auto"]:
        log_ent_coef = torch.tensor([c["log_ent_coef"]], dtype=dtype, device=device, requires_grad=True)
        ent_coef = torch.exp(log_ent_coef.detach())                                                         # :311
        ent_coef_loss = -(log_ent_coef * (log_prob + c["target_entropy"]).detach()).mean()                  # :312
        ent_coef_loss.backward()                                                                            # :323
        out["ent_coef_loss"] = n64(ent_coef_loss)
        grad["log_ent_coef"] = n64(log_ent_coef.grad)
    else:
        ent_coef = torch.tensor(c["ent_coef"], dtype=dtype, device=device)                                  # :315
    with torch.no_grad():                                                                                   # :326-335
        nxt = actor_forward(P, t("x_next"), t("noise_next"), stable)
        q_next, pre_t = critic_forward(P, "critic_target", t("x_next"), nxt["actions"])
        next_q = torch.min(q_next.t(), dim=1, keepdim=True)[0]
        next_q = next_q - ent_coef * nxt["log_prob"].reshape(-1, 1)
        target_q = t("rewards").reshape(-1, 1) + (1 - t("dones").reshape(-1, 1)) * c["gamma"] * next_q
    q_replay, pre_r = critic_forward(P, "critic", x, t("a_replay"))                                         # :339
    critic_loss = 0.5 * sum(F.mse_loss(q.reshape(-1, 1), target_q) for q in q_replay)                       # :342
    critic_loss.backward()                                                                                  # :348
    for k, p in P.items():
        if k.startswith("critic."):
            grad[k] = n64(p.grad)
            p.grad = None                                                                                   # :347 of the next step
    q_pi, pre_p = critic_forward(P, "critic", x, a_pi)                                                      # :354
    min_q = torch.min(q_pi.t(), dim=1, keepdim=True)[0]                                                     # :355
    actor_loss = (ent_coef * log_prob - min_q).mean()                                                       # :356
    actor_loss.backward()                                                                                   # :361
    for k, p in P.items():
        if k.startswith("actor."):
            grad[k] = n64(p.grad)
    grad["x"] = n64(x.grad)
    out["grad_critic_from_actor_loss"] = {k: n64(p.grad) for k, p in P.items() if k.startswith("critic.")}
    target = {}
    with torch.no_grad():                                                                                   # :366, SB3's polyak_update
        for k, p in P.items():
            if k.startswith("critic_target."):
                target[k] = n64((1 - c["tau"]) * p + c["tau"] * P["critic." + k[len("critic_target."):]])
    out.update(a_pi=n64(a_pi), log_prob=n64(log_prob).ravel(), ent_coef=n64(ent_coef).ravel()[0], target_q=n64(target_q).ravel(),
               q_replay=n64(q_replay), critic_loss=n64(critic_loss), q_pi=n64(q_pi), actor_loss=n64(actor_loss), grad=grad, target=target,
               a_next=n64(nxt["actions"]), log_prob_next=n64(nxt["log_prob"]), q_next=n64(q_next),
               pre=[n64(p) for p in act["pre"] + nxt["pre"] + pre_t + pre_r + pre_p], s_pre=[n64(act["s_pre"]), n64(nxt["s_pre"])],
               u=[n64(act["u"]), n64(nxt["u"])])
    return out


def conditions(ref):
    """The distances the comparisons rest on, from a float64 step_ref."""
    pre = np.concatenate([p.ravel() for p in ref["pre"]]) if ref["pre"] else np.zeros(0)
    s = np.concatenate([p.ravel() for p in ref["s_pre"]])
    return dict(gate=float(np.abs(pre).min()) if pre.size else float("inf"),
                tie=float(min(np.abs(ref["q_next"][0] - ref["q_next"][1]).min(), np.abs(ref["q_pi"][0] - ref["q_pi"][1]).min())),
                clamp=float(np.minimum(np.abs(s - LOG_STD_MIN), np.abs(s - LOG_STD_MAX)).min()),
                saturated=float((np.abs(pre) > 2).mean()) if pre.size else None, above_clamp=float((s > LOG_STD_MAX).mean()),
                u_max=float(max(np.abs(u).max() for u in ref["u"])))


def make_params(arch, seed, hi):
    """{name: float64 tensor}: trained-like parameters of a head (see the module docstring)."""
    Fd, pi, qf, A = arch
    g = torch.Generator().manual_seed(seed)
    rn = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)      # noqa: E731
    x = rn(512, Fd)
    P = {}
    h = x
    for l, w in enumerate(pi):
        W, b = rn(w, h.shape[1]), 0.2 * rn(w)
        W = W * (PRE_STD / float(F.linear(h, W).std()))
        P[f"actor.latent_pi.{2 * l}.weight"], P[f"actor.latent_pi.{2 * l}.bias"] = W, b
        h = torch.relu(F.linear(h, W, b))
    W = rn(A, h.shape[1])
    P["actor.mu.weight"], P["actor.mu.bias"] = W * (1.3 / float(F.linear(h, W).std())), 0.1 * rn(A)
    W = rn(A, h.shape[1])
    W = W * (0.5 / float(F.linear(h, W).std()))
    P["actor.log_std.weight"] = W
    P["actor.log_std.bias"] = (1.7 if hi else -1.0) - F.linear(h, W).mean(0) + 0.1 * rn(A)
    xa = torch.cat([x, torch.tanh(1.5 * rn(512, A))], dim=1)
    for prefix in ("critic", "critic_target"):
        for c in range(2):
            h = xa
            for l, w in enumerate(qf):
                W, b = rn(w, h.shape[1]), 0.2 * rn(w)
                W = W * (PRE_STD / float(F.linear(h, W).std()))
                if prefix == "critic_target":          # a target that trails its critic
                    W = 0.9 * P[f"critic.qf{c}.{2 * l}.weight"] + 0.1 * W
                    b = 0.9 * P[f"critic.qf{c}.{2 * l}.bias"] + 0.1 * b
                P[f"{prefix}.qf{c}.{2 * l}.weight"], P[f"{prefix}.qf{c}.{2 * l}.bias"] = W, b
                h = torch.relu(F.linear(h, W, b))
            W, b = rn(1, h.shape[1]), 0.5 * rn(1)
            W = W * (2.0 / float(F.linear(h, W).std()))
            if prefix == "critic_target":
                W = 0.9 * P[f"critic.qf{c}.{2 * len(qf)}.weight"] + 0.1 * W
                b = 0.9 * P[f"critic.qf{c}.{2 * len(qf)}.bias"] + 0.1 * b
            P[f"{prefix}.qf{c}.{2 * len(qf)}.weight"], P[f"{prefix}.qf{c}.{2 * len(qf)}.bias"] = W, b
    return {k: P[k] for k in param_names(arch)}


def _pre_owner(arch):
    """The bias behind each entry of step_ref's `pre` list, in its order: actor at x, actor at x', target critics, critics twice."""
    _, pi, qf, _ = arch
    actor = [f"actor.latent_pi.{2 * l}.bias" for l in range(len(pi))]
    crit = lambda prefix: [f"{prefix}.qf{c}.{2 * l}.bias" for c in range(2) for l in range(len(qf))]      # noqa: E731
    return actor + actor + crit("critic_target") + crit("critic") + crit("critic")


def settle(c, rounds=200):
    """Nudge biases (by a few margins at a time, in float32 steps) until the input conditions of the module docstring hold in float64."""
    owners = _pre_owner(c["arch"])
    nq = len(c["arch"][2])
    for _ in range(rounds):
        ref = step_ref(c)
        moved = False
        P = c["params"]
        for name, pre in zip(owners, ref["pre"]):
            bad = (np.abs(pre) < 1.5 * GATE_MARGIN).any(axis=0)
            if bad.any():
                P[name] = (P[name] + np.where(bad, 4 * GATE_MARGIN, 0.0)).astype(np.float32)
                moved = True
        for s in ref["s_pre"]:
            bad = (np.minimum(np.abs(s - LOG_STD_MIN), np.abs(s - LOG_STD_MAX)) < 1.5 * CLAMP_MARGIN).any(axis=0)
            if bad.any():
                P["actor.log_std.bias"] = (P["actor.log_std.bias"] + np.where(bad, 4 * CLAMP_MARGIN, 0.0)).astype(np.float32)
                moved = True
        for prefix, q in (("critic_target", ref["q_next"]), ("critic", ref["q_pi"])):
            if (np.abs(q[0] - q[1]) < 1.5 * TIE_MARGIN).any():
                P[f"{prefix}.qf1.{2 * nq}.bias"] = (P[f"{prefix}.qf1.{2 * nq}.bias"] + 8 * TIE_MARGIN).astype(np.float32)
                moved = True
        if not moved:
            return c
    raise AssertionError("the input conditions did not settle")


def make_inputs(arch, B, hi, auto, seed):
    """One replay batch for a head: parameters, features of both observations, the two noise draws, replay actions, rewards, dones (both 0 and 1
    when B > 1) and the step's constants.  float32 numpy arrays, settled."""
    Fd, pi, qf, A = arch
    P = {k: v.float().numpy() for k, v in make_params(arch, seed, hi).items()}
    g = torch.Generator().manual_seed(seed + 1)
    rn = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64).float().numpy()      # noqa: E731
    dones = (torch.rand(B, generator=g) < 0.3).float().numpy()
    if B > 1:
        dones[0], dones[1] = 0.0, 1.0
    c = dict(params=P, x=rn(B, Fd), x_next=rn(B, Fd), noise_pi=rn(B, A), noise_next=rn(B, A), a_replay=np.tanh(1.5 * rn(B, A)).astype(np.float32),
             rewards=rn(B), dones=dones, gamma=GAMMA, tau=TAU, auto=auto, log_ent_coef=float(np.float32(math.log(0.2))), ent_coef=0.15,
             target_entropy=-float(A), arch=arch, hi=hi)
    return settle(c)


@lru_cache(maxsize=None)
def gpu_case(name):
    arch, B, hi, auto = GPU_CASES[name]
    return make_inputs(ARCHS[arch], B, hi, auto, seed=2000 + sorted(GPU_CASES).index(name))


@lru_cache(maxsize=None)
def gpu_reference(name):
    return step_ref(gpu_case(name))


def actor_ref(c, dactions, dlogp, which="x", dtype=torch.float64):
    """action_log_prob alone at x (or x_next) with given output gradients: outputs, and the gradients in the features and the actor's parameters."""
    P = as_torch(c["params"], dtype)
    x = torch.from_numpy(c[which]).to(dtype).requires_grad_(True)
    o = actor_forward(P, x, torch.from_numpy(c["noise_pi" if which == "x" else "noise_next"]).to(dtype))
    ((o["actions"] * torch.from_numpy(dactions).to(dtype)).sum() + (o["log_prob"] * torch.from_numpy(dlogp).to(dtype)).sum()).backward()
    n64 = lambda v: v.detach().double().numpy()      # noqa: E731
    grad = {"x": n64(x.grad)}
    grad.update({k: n64(p.grad) for k, p in P.items() if k.startswith("actor.")})
    return dict(actions=n64(o["actions"]), log_prob=n64(o["log_prob"]), mu=n64(o["mu"]), grad=grad)


def critic_ref(c, actions, dq, prefix="critic", dtype=torch.float64):
    """q_values alone at (x, actions) with a given output gradient: q (2, B), and the gradients in the actions and the critics' parameters."""
    P = {k: v.detach().requires_grad_(True) for k, v in as_torch(c["params"], dtype).items()}
    a = torch.from_numpy(actions).to(dtype).requires_grad_(True)
    x = torch.from_numpy(c["x"]).to(dtype).requires_grad_(True)
    q, _ = critic_forward(P, prefix, x, a)
    (q * torch.from_numpy(dq).to(dtype)).sum().backward()
    n64 = lambda v: v.detach().double().numpy()      # noqa: E731
    assert x.grad is None
    grad = {"actions": n64(a.grad)}
    grad.update({k: n64(p.grad) for k, p in P.items() if k.startswith(prefix + ".")})
    return dict(q=n64(q), grad=grad)
