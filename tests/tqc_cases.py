"""Float64 restatement of the TQC head (include/m3l_amd.h "SAC TQC critics", m3l_amd/tqc.py) and the inputs of its tests (test_tqc_cpu.py,
test_tqc_gpu.py, tools/sac_head_bench.py), built on sac_ens_cases: the actor, the batch, the hidden layers of the N critics and the margins
are its; the last Linear of every critic is replaced by one with n_quantiles outputs.

The rule, written as sb3-contrib writes it (`TQC.train`, `Critic`, `quantile_huber_loss`; restated from memory, sb3-contrib is not part of the
reference tree: PARITY UNPINNED): the target critics' quantiles at (x', a') are pooled per row, `torch.sort`ed and cut to `[:, :K]`; the loss is
the 4-D broadcast of targets against current quantiles under the Huber function and |tau - [delta < 0]|, `.mean()` over everything.

What the float32 / float64 comparisons rest on: the loss, its gradient in z and the sorted values are continuous in every input (clamp(delta)
is 0 where the indicator jumps, Huber is C1 at |delta| = 1), so nothing is asked of delta; the ReLU gates of the nets are settled by
sac_ens_cases.settle at every point where a gradient is taken ((x, a_replay) and (x, a_pi)): they do not depend on the last layer."""
from functools import lru_cache

import numpy as np
import torch
from torch import nn
from torch.nn import functional as F

import sac_cases as SC
import sac_ens_cases as EC

PI = (32,)
# name -> (features, qf widths, actions, N, n_quantiles, top_quantiles_to_drop_per_net, B)
CASES = {
    "f16_a1_nohid_n1q1d0_b1": (16, (), 1, 1, 1, 0, 1),              # the smallest of everything
    "f32_a7_q32_n1q1d0_b17": (32, (32,), 7, 1, 1, 0, 17),           # one quantile: the ensemble's critic (the anchor)
    "f32_a7_q32_n2q25d2_b17": (32, (32,), 7, 2, 25, 2, 17),         # sb3-contrib's defaults, a ragged second tile
    "f32_a7_nohid_n2q25d2_b37": (32, (), 7, 2, 25, 2, 37),          # the head straight off cat([x, a]): the EDGE form, 25 rows of 39
    "f16_a7_q48x32_n3q5d4_b37": (16, (48, 32), 7, 3, 5, 4, 37),     # one quantile kept per net, three tiles
    "f16_a1_q32_n3q5d4_b1": (16, (32,), 1, 3, 5, 4, 1),
    "f32_a1_q48x32_n2q64d0_b37": (32, (48, 32), 1, 2, 64, 0, 37),   # the full head tile, nothing dropped
    "f16_a1_nohid_n2q64d0_b17": (16, (), 1, 2, 64, 0, 17),
    "f32_a7_q48x32_n5q7d3_b17": (32, (48, 32), 7, 5, 7, 3, 17),     # 15 Linears: two weight-gradient launches
    "f16_a7_q32_n10q25d2_b17": (16, (32,), 7, 10, 25, 2, 17),       # the largest pool of the grid, 250
    "f32_a7_q48x32_n2q25d2_b37": (32, (48, 32), 7, 2, 25, 2, 37),   # the whole step
}
STEP = "f32_a7_q48x32_n2q25d2_b37"
ANCHOR = "f32_a7_q32_n1q1d0_b17"


def arch_of(name):
    Fd, qf, A = CASES[name][:3]
    return (Fd, PI, tuple(qf), A)


def kept(N, nq, d):
    """K: the target quantiles kept per row."""
    return N * (nq - d)


critic_names, param_names, ent_of, polyak_ref = EC.critic_names, EC.param_names, EC.ent_of, EC.polyak_ref


def make_heads(arch, N, nq, seed):
    """{name: float32 array} of the last Linear of every critic and target critic: quantile-like outputs (a spread of biases under outputs of
    standard deviation about 1), the target 0.9 critic + 0.1 fresh."""
    Fd, _, qf, A = arch
    k = qf[-1] if qf else Fd + A
    g = torch.Generator().manual_seed(seed)
    rn = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)      # noqa: E731
    P = {}
    for prefix in ("critic", "critic_target"):
        for c in range(N):
            W = rn(nq, k) * (1.0 / (0.8 * k) ** 0.5)
            b = 0.5 * rn(nq) + torch.linspace(-1.0, 1.0, nq, dtype=torch.float64) * (nq > 1)
            if prefix == "critic_target":
                W, b = 0.9 * P[f"critic.qf{c}.{2 * len(qf)}.weight"] + 0.1 * W, 0.9 * P[f"critic.qf{c}.{2 * len(qf)}.bias"] + 0.1 * b
            P[f"{prefix}.qf{c}.{2 * len(qf)}.weight"], P[f"{prefix}.qf{c}.{2 * len(qf)}.bias"] = W, b
    return {k_: v.float().numpy() for k_, v in P.items()}


def make_inputs(arch, N, nq, d, B, seed):
    """sac_ens_cases.make_inputs' settled batch, actor and N critics with heads of nq outputs.  float32 numpy arrays."""
    c = dict(EC.make_inputs(arch, N, B, seed))
    c["params"] = dict(c["params"])
    c["params"].update(make_heads(arch, N, nq, seed + 5))
    c["n_quantiles"], c["drop"], c["K"] = nq, d, kept(N, nq, d)
    return c


@lru_cache(maxsize=None)
def case(name):
    Fd, qf, A, N, nq, d, B = CASES[name]
    return make_inputs(arch_of(name), N, nq, d, B, seed=7000 + 10 * sorted(CASES).index(name))


def as_modules(c, dtype=torch.float64):
    """The nets as torch.nn modules under the head's names: actor.latent_pi / mu / log_std, critic.qf{i} and critic_target.qf{i}, each qf a
    Sequential of Linear + ReLU pairs and a last Linear(., n_quantiles), loaded from the case's parameters."""
    Fd, pi, qf, A = c["arch"]

    def seq(k, widths, out=None):
        mods = []
        for w in widths:
            mods += [nn.Linear(k, w), nn.ReLU()]
            k = w
        return nn.Sequential(*mods, *([nn.Linear(k, out)] if out is not None else [])), k
    m = nn.Module()
    m.actor = nn.Module()
    m.actor.latent_pi, k = seq(Fd, pi)
    m.actor.mu, m.actor.log_std = nn.Linear(k, A), nn.Linear(k, A)
    for name in ("critic", "critic_target"):
        sub = nn.Module()
        for i in range(c["n_critics"]):
            setattr(sub, f"qf{i}", seq(Fd + A, qf, c["n_quantiles"])[0])
        setattr(m, name, sub)
    m.load_state_dict({k_: torch.from_numpy(np.asarray(v)) for k_, v in c["params"].items()}, strict=True)
    return m.to(dtype)


def critic_forward(P, prefix, x, actions, N):
    """sb3-contrib's Critic with N nets and a shared extractor: the features enter detached.  -> quantiles (N, B, nq) (sb3-contrib stacks them
    as (B, N, nq); this is the head's public layout), the ReLU pre-activations (critic-major)."""
    xa = torch.cat([x.detach(), actions], dim=1)
    zs, pres = [], []
    for c in range(N):
        h, l = xa, 0
        while f"{prefix}.qf{c}.{2 * l + 2}.weight" in P:
            pre = F.linear(h, P[f"{prefix}.qf{c}.{2 * l}.weight"], P[f"{prefix}.qf{c}.{2 * l}.bias"])
            pres.append(pre)
            h = torch.relu(pre)
            l += 1
        zs.append(F.linear(h, P[f"{prefix}.qf{c}.{2 * l}.weight"], P[f"{prefix}.qf{c}.{2 * l}.bias"]))
    return torch.stack(zs), pres


def truncated_target(z_next, log_prob_next, rewards, dones, gamma, ent, K):
    """sb3-contrib's target: z_next (N, B, nq) -> (B, N nq) pooled, sorted, [:, :K], the entropy term, the Bellman line -> (B, K)."""
    B = z_next.shape[1]
    pooled = z_next.permute(1, 0, 2).reshape(B, -1)
    sorted_z, _ = torch.sort(pooled)
    t = sorted_z[:, :K] - ent * log_prob_next.reshape(-1, 1)
    return rewards.reshape(-1, 1) + (1 - dones.reshape(-1, 1)) * torch.as_tensor(gamma, dtype=t.dtype, device=t.device).reshape(-1, 1) * t


def quantile_huber_loss(z, target, weights=None):
    """sb3-contrib's quantile_huber_loss with sum_over_quantiles=False: z (N, B, nq) current, target (B, K); the 4-D broadcast, `.mean()`."""
    cur = z.permute(1, 0, 2)                                                        # (B, N, nq)
    nq = cur.shape[-1]
    cum_prob = ((torch.arange(nq, dtype=cur.dtype, device=cur.device) + 0.5) / nq).view(1, 1, -1, 1)
    delta = target.unsqueeze(1).unsqueeze(1) - cur.unsqueeze(-1)                    # (B, N, nq, K)
    a = delta.abs()
    huber = torch.where(a > 1, a - 0.5, delta ** 2 * 0.5)
    loss = torch.abs(cum_prob - (delta.detach() < 0).to(cur.dtype)) * huber
    if weights is not None:
        loss = loss * weights.view(-1, 1, 1, 1)
    return loss.mean()


def forward_ref(c, dtype=torch.float64, noise_next=None):
    """Every forward value of a step, without a tape -> float64 numpy: a_pi, log_prob, a_next, log_prob_next, z_next (the N target critics at
    (x', a')), z_replay, z_pi, and the ReLU pre-activations at the points where the tests take gradients."""
    P = SC.as_torch(c["params"], dtype)
    t = lambda k: torch.from_numpy(c[k]).to(dtype)      # noqa: E731
    N = c["n_critics"]
    n64 = lambda v: v.detach().double().numpy()      # noqa: E731
    nn_ = t("noise_next") if noise_next is None else torch.from_numpy(noise_next).to(dtype)
    with torch.no_grad():
        act = SC.actor_forward(P, t("x"), t("noise_pi"), stable=dtype != torch.float64)
        nxt = SC.actor_forward(P, t("x_next"), nn_, stable=dtype != torch.float64)
        z_next, _ = critic_forward(P, "critic_target", t("x_next"), nxt["actions"], N)
        z_replay, pre_r = critic_forward(P, "critic", t("x"), t("a_replay"), N)
        z_pi, pre_p = critic_forward(P, "critic", t("x"), act["actions"], N)
    return dict(a_pi=n64(act["actions"]), log_prob=n64(act["log_prob"]), a_next=n64(nxt["actions"]), log_prob_next=n64(nxt["log_prob"]),
                z_next=n64(z_next), z_replay=n64(z_replay), z_pi=n64(z_pi), pre=[n64(p) for p in act["pre"] + pre_r + pre_p])


@lru_cache(maxsize=None)
def reference(name):
    return forward_ref(case(name))


def target_ref(c, gamma, ent, noise_next=None):
    """target (B, K) in float64; gamma a number or (B,); noise_next: another draw for the actor at x' (zeros: the deterministic action)."""
    ref = forward_ref(c, noise_next=noise_next)
    f = lambda v: torch.from_numpy(np.array(v, dtype=np.float64))      # noqa: E731
    g = np.broadcast_to(np.asarray(gamma, dtype=np.float64), c["rewards"].shape)
    return truncated_target(f(ref["z_next"]), f(ref["log_prob_next"]), f(c["rewards"]), f(c["dones"]), f(g), ent, c["K"]).numpy()


def z_ref(c, actions, dz, prefix="critic"):
    """quantiles alone at (x, actions) with a given output gradient (N, B, nq): z, and the gradients in the actions and the critics' parameters."""
    P = {k: v.detach().requires_grad_(True) for k, v in SC.as_torch(c["params"]).items()}
    a = torch.from_numpy(actions).double().requires_grad_(True)
    x = torch.from_numpy(c["x"]).double().requires_grad_(True)
    z, _ = critic_forward(P, prefix, x, a, c["n_critics"])
    (z * torch.from_numpy(dz).double()).sum().backward()
    assert x.grad is None
    n64 = lambda v: v.detach().double().numpy()      # noqa: E731
    grad = {"actions": n64(a.grad)}
    grad.update({k: n64(p.grad) for k, p in P.items() if k.startswith(prefix + ".")})
    return dict(z=n64(z), grad=grad)


def critic_loss_ref(c, target, weights=None, dtype=torch.float64):
    """The quantile-Huber loss of the N critics at (x, a_replay) against a given target (B, K): loss, td_abs = the row's mean |delta|,
    coef = d loss / d z, and the gradient of every critic parameter."""
    P = SC.as_torch(c["params"], dtype)
    z, _ = critic_forward(P, "critic", torch.from_numpy(c["x"]).to(dtype), torch.from_numpy(c["a_replay"]).to(dtype), c["n_critics"])
    z.retain_grad()
    t = torch.from_numpy(np.asarray(target, dtype=np.float64)).to(dtype)
    w = None if weights is None else torch.from_numpy(np.asarray(weights)).to(dtype)
    loss = quantile_huber_loss(z, t, w)
    loss.backward()
    n64 = lambda v: v.detach().double().numpy()      # noqa: E731
    td = (t.unsqueeze(1).unsqueeze(1) - z.detach().permute(1, 0, 2).unsqueeze(-1)).abs().mean(dim=(1, 2, 3))
    return dict(loss=n64(loss), td_abs=n64(td), coef=n64(z.grad), grad={k: n64(p.grad) for k, p in P.items() if k.startswith("critic.")})


def actor_loss_ref(c, ent, dtype=torch.float64):
    """mean_b (ent logp - mean_{c, j} z[c, b, j](x, a_pi)): the loss, log_prob, and the gradients of the actor's parameters and of x."""
    P = SC.as_torch(c["params"], dtype)
    x = torch.from_numpy(c["x"]).to(dtype).requires_grad_(True)
    act = SC.actor_forward(P, x, torch.from_numpy(c["noise_pi"]).to(dtype), stable=dtype != torch.float64)
    z, _ = critic_forward(P, "critic", x, act["actions"], c["n_critics"])
    loss = (ent * act["log_prob"] - z.mean(dim=(0, 2))).mean()
    loss.backward()
    n64 = lambda v: v.detach().double().numpy()      # noqa: E731
    grad = {k: n64(p.grad) for k, p in P.items() if k.startswith("actor.")}
    grad["x"] = n64(x.grad)
    return dict(loss=n64(loss), log_prob=n64(act["log_prob"]), grad=grad)
