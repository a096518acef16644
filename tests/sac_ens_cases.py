"""Float64 restatement of the SAC critic ensemble (include/m3l_amd.h "SAC critic ensemble", m3l_amd/sac_ensemble.py) and the inputs of its tests
(test_sac_ens_cpu.py, test_sac_ens_gpu.py, tools/sac_head_bench.py), built on sac_cases: the actor, the inputs' scaling and the margins are
its; the critics are N nets made by its recipe.

The rule, from torch primitives (nn.functional.linear, torch.relu, autograd): N critics over cat([x, a]); the TD target's minimum over a subset
of the target critics (REDQ, Chen et al. 2021); SB3's critic loss summed over the critics, with importance weights and the mean absolute TD
error; the actor loss against min_c q_c (SB3's n_critics semantics) or mean_c q_c (REDQ).  Neither SB3 nor a REDQ implementation is part of the
reference tree: PARITY UNPINNED.  At N = 2, subset None and the min reduction it is sac_cases.step_ref, which test_sac_ens_cpu.py asserts.

`settle` nudges biases until, in float64, over every evaluation the tests make (the actor at x and x', all N critics at (x, a_replay) and
(x, a_pi), all N target critics at (x', a')):
  * every ReLU pre-activation has |pre| >= GATE_MARGIN;
  * on every row the two smallest values among the target critics of every subset of the case, and among all N critics at (x, a_pi), differ by
    at least TIE_MARGIN;
  * no pre-clamp log_std lies within CLAMP_MARGIN of an edge (the actor is sac_cases' and arrives settled; it is checked again)."""
from functools import lru_cache

import numpy as np
import torch
from torch.nn import functional as F

import sac_cases as SC

MAX_CRITICS = 10

# name -> (arch of sac_cases.ARCHS, N, B)
CASES = {
    "a64_n1_b17": ("a64", 1, 17),
    "a64_n2_b33": ("a64", 2, 33),            # the anchor
    "a64_n3_b17": ("a64", 3, 17),            # odd N: a second, partly filled weight-gradient launch
    "a64_n10_b33": ("a64", 10, 33),          # the maximum
    "mixed_n3_b33": ("mixed", 3, 33),        # 4 Linears per critic, A = 1: 12 Linears in 2 launches
    "mixed_n5_b1": ("mixed", 5, 1),
    "nohid_n10_b3": ("nohid", 10, 3),
    "amax_n3_b17": ("amax", 3, 17),          # no hidden critic layer: the edge-path head; A = 64
}
ANCHOR = "a64_n2_b33"


def subsets(N):
    """The subsets every case is run with: all, the first, the last, two distinct entries in descending order, a list with a duplicate."""
    out = [None, [0], [N - 1]]
    if N >= 2:
        out += [[N - 1, 0], [N - 1, N - 1]]
    if N >= 3:
        out += [[1, N - 1, 1]]
    return out


def critic_names(arch, N, prefix="critic"):
    """State-dict names of the N critics in SACEnsembleParams.critic_flat order."""
    return [f"{prefix}.qf{c}.{2 * l}.{t}" for c in range(N) for l in range(len(arch[2]) + 1) for t in ("weight", "bias")]


def param_names(arch, N):
    """Every name of a SACEnsembleHead's state dict, in creation order."""
    return SC.actor_names(arch) + critic_names(arch, N) + critic_names(arch, N, "critic_target")


def critic_forward(P, prefix, x, actions, N):
    """SB3's ContinuousCritic with N nets and a shared extractor: the features enter detached.  -> q (N, B), the ReLU pre-activations (critic-major)."""
    xa = torch.cat([x.detach(), actions], dim=1)
    qs, pres = [], []
    for c in range(N):
        h, l = xa, 0
        while f"{prefix}.qf{c}.{2 * l + 2}.weight" in P:
            pre = F.linear(h, P[f"{prefix}.qf{c}.{2 * l}.weight"], P[f"{prefix}.qf{c}.{2 * l}.bias"])
            pres.append(pre)
            h = torch.relu(pre)
            l += 1
        qs.append(F.linear(h, P[f"{prefix}.qf{c}.{2 * l}.weight"], P[f"{prefix}.qf{c}.{2 * l}.bias"]).flatten())
    return torch.stack(qs), pres


def make_critics(arch, N, seed):
    """{name: float64 tensor}: N critics and their trailing targets by sac_cases.make_params' recipe (pre-activations of standard deviation
    PRE_STD, q of standard deviation 2, a target 0.9 critic + 0.1 fresh)."""
    Fd, _, qf, A = arch
    g = torch.Generator().manual_seed(seed)
    rn = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)      # noqa: E731
    xa = torch.cat([rn(512, Fd), torch.tanh(1.5 * rn(512, A))], dim=1)
    P = {}
    for prefix in ("critic", "critic_target"):
        for c in range(N):
            h = xa
            for l, w in enumerate(tuple(qf) + (1,)):
                last = l == len(qf)
                W, b = rn(w, h.shape[1]), (0.5 if last else 0.2) * rn(w)
                W = W * ((2.0 if last else SC.PRE_STD) / float(F.linear(h, W).std()))
                if prefix == "critic_target":
                    W = 0.9 * P[f"critic.qf{c}.{2 * l}.weight"] + 0.1 * W
                    b = 0.9 * P[f"critic.qf{c}.{2 * l}.bias"] + 0.1 * b
                P[f"{prefix}.qf{c}.{2 * l}.weight"], P[f"{prefix}.qf{c}.{2 * l}.bias"] = W, b
                h = torch.relu(F.linear(h, W, b))
    return P


def forward_ref(c, dtype=torch.float64):
    """Every forward value of a step, without a tape -> float64 numpy: a_pi, log_prob, a_next, log_prob_next, q_next (the N target critics at
    (x', a')), q_replay, q_pi, and the quantities of the input conditions (pre: owner-ordered as `_pre_owner`)."""
    P = SC.as_torch(c["params"], dtype)
    t = lambda k: torch.from_numpy(c[k]).to(dtype)      # noqa: E731
    N = c["n_critics"]
    n64 = lambda v: v.detach().double().numpy()      # noqa: E731
    with torch.no_grad():
        act = SC.actor_forward(P, t("x"), t("noise_pi"), stable=dtype != torch.float64)
        nxt = SC.actor_forward(P, t("x_next"), t("noise_next"), stable=dtype != torch.float64)
        q_next, pre_t = critic_forward(P, "critic_target", t("x_next"), nxt["actions"], N)
        q_replay, pre_r = critic_forward(P, "critic", t("x"), t("a_replay"), N)
        q_pi, pre_p = critic_forward(P, "critic", t("x"), act["actions"], N)
    return dict(a_pi=n64(act["actions"]), log_prob=n64(act["log_prob"]), a_next=n64(nxt["actions"]), log_prob_next=n64(nxt["log_prob"]),
                q_next=n64(q_next), q_replay=n64(q_replay), q_pi=n64(q_pi), pre=[n64(p) for p in act["pre"] + nxt["pre"] + pre_t + pre_r + pre_p],
                s_pre=[n64(act["s_pre"]), n64(nxt["s_pre"])], u=[n64(act["u"]), n64(nxt["u"])])


def _pre_owner(arch, N):
    """The bias behind each entry of forward_ref's `pre` list."""
    _, pi, qf, _ = arch
    actor = [f"actor.latent_pi.{2 * l}.bias" for l in range(len(pi))]
    crit = lambda prefix: [f"{prefix}.qf{c}.{2 * l}.bias" for c in range(N) for l in range(len(qf))]      # noqa: E731
    return actor + actor + crit("critic_target") + crit("critic") + crit("critic")


def two_smallest_gap(q):
    """q (M, B), M >= 2 -> per row the distance between the two smallest of the M values."""
    s = np.sort(q, axis=0)
    return s[1] - s[0]


def tie_gaps(ref, N):
    """{what: smallest gap over the rows} for every minimum the tests take: each subset's target critics (distinct entries), all N at (x, a_pi)."""
    out = {}
    for sub in subsets(N):
        idx = sorted(set(range(N) if sub is None else sub))
        if len(idx) >= 2:
            out[f"target {sub}"] = float(two_smallest_gap(ref["q_next"][idx]).min())
    if N >= 2:
        out["q_pi"] = float(two_smallest_gap(ref["q_pi"]).min())
    return out


def conditions(ref, N):
    pre = np.concatenate([p.ravel() for p in ref["pre"]]) if ref["pre"] else np.zeros(0)
    s = np.concatenate([p.ravel() for p in ref["s_pre"]])
    gaps = tie_gaps(ref, N)
    return dict(gate=float(np.abs(pre).min()) if pre.size else float("inf"), tie=min(gaps.values()) if gaps else float("inf"),
                clamp=float(np.minimum(np.abs(s - SC.LOG_STD_MIN), np.abs(s - SC.LOG_STD_MAX)).min()))


def settle(c, rounds=200):
    """Nudge biases (by a few margins at a time, in float32 steps) until the input conditions of the module docstring hold in float64."""
    arch, N = c["arch"], c["n_critics"]
    owners = _pre_owner(arch, N)
    nq = len(arch[2])
    P = c["params"]
    for _ in range(rounds):
        ref = forward_ref(c)
        moved = False
        for name, pre in zip(owners, ref["pre"]):
            bad = (np.abs(pre) < 1.5 * SC.GATE_MARGIN).any(axis=0)
            if bad.any():
                P[name] = (P[name] + np.where(bad, 4 * SC.GATE_MARGIN, 0.0)).astype(np.float32)
                moved = True
        for s in ref["s_pre"]:
            bad = (np.minimum(np.abs(s - SC.LOG_STD_MIN), np.abs(s - SC.LOG_STD_MAX)) < 1.5 * SC.CLAMP_MARGIN).any(axis=0)
            if bad.any():
                P["actor.log_std.bias"] = (P["actor.log_std.bias"] + np.where(bad, 4 * SC.CLAMP_MARGIN, 0.0)).astype(np.float32)
                moved = True
        for prefix, q in (("critic_target", ref["q_next"]), ("critic", ref["q_pi"])):
            for i in range(N):          # the later critic of a close pair moves
                for j in range(i + 1, N):
                    if (np.abs(q[i] - q[j]) < 1.5 * SC.TIE_MARGIN).any():
                        P[f"{prefix}.qf{j}.{2 * nq}.bias"] = (P[f"{prefix}.qf{j}.{2 * nq}.bias"] + 8 * SC.TIE_MARGIN).astype(np.float32)
                        moved = True
        if not moved:
            return c
    raise AssertionError("the input conditions did not settle")


def make_inputs(arch, N, B, seed, hi=False, auto=True):
    """sac_cases.make_inputs' batch and actor with N critics in place of its two, settled again.  float32 numpy arrays."""
    c = dict(SC.make_inputs(arch, B, hi, auto, seed))
    P = {k: v for k, v in c["params"].items() if k.startswith("actor.")}
    P.update({k: v.float().numpy() for k, v in make_critics(arch, N, seed + 2).items()})
    c["params"] = {k: P[k] for k in param_names(arch, N)}
    c["n_critics"] = N
    g = torch.Generator().manual_seed(seed + 3)
    c["weights"] = (0.25 + 1.5 * torch.rand(B, generator=g)).float().numpy()                       # importance weights of a prioritised batch
    c["discounts"] = (SC.GAMMA ** (1 + torch.arange(B) % 3).double()).float().numpy()              # of an n-step batch, n = 3
    return settle(c)


@lru_cache(maxsize=None)
def case(name):
    arch, N, B = CASES[name]
    return make_inputs(SC.ARCHS[arch], N, B, seed=4000 + 10 * sorted(CASES).index(name))


@lru_cache(maxsize=None)
def reference(name):
    return forward_ref(case(name))


def ent_of(c):
    """The fixed entropy coefficient the tests hand over as a number, and as the logarithm whose exp the kernels take."""
    return float(np.exp(np.float64(c["log_ent_coef"])))


def target_ref(c, ref, subset, gamma, ent):
    """target_q (B,) in float64: r + (1 - done) g (min over the subset of q_target_c(x', a') - ent logp'); gamma a number or (B,)."""
    N = c["n_critics"]
    idx = list(range(N)) if subset is None else list(subset)
    nq = ref["q_next"][idx].min(axis=0) - ent * ref["log_prob_next"]
    return c["rewards"].astype(np.float64) + (1.0 - c["dones"].astype(np.float64)) * np.asarray(gamma, dtype=np.float64) * nq


def q_ref(c, actions, dq, prefix="critic"):
    """q_values alone at (x, actions) with a given output gradient (N, B): q, and the gradients in the actions and the critics' parameters."""
    N = c["n_critics"]
    P = {k: v.detach().requires_grad_(True) for k, v in SC.as_torch(c["params"]).items()}
    a = torch.from_numpy(actions).double().requires_grad_(True)
    x = torch.from_numpy(c["x"]).double().requires_grad_(True)
    q, _ = critic_forward(P, prefix, x, a, N)
    (q * torch.from_numpy(dq).double()).sum().backward()
    assert x.grad is None
    n64 = lambda v: v.detach().double().numpy()      # noqa: E731
    grad = {"actions": n64(a.grad)}
    grad.update({k: n64(p.grad) for k, p in P.items() if k.startswith(prefix + ".")})
    return dict(q=n64(q), grad=grad)


def critic_loss_ref(c, target_q, weights=None):
    """SB3's critic loss for N critics at (x, a_replay) against a given target: loss = 0.5 sum_c mean_r w_r (q_c - t)^2, td_abs = mean_c |q_c - t|,
    coef = d loss / d q, and the gradient of every critic parameter."""
    N = c["n_critics"]
    P = SC.as_torch(c["params"])
    q, _ = critic_forward(P, "critic", torch.from_numpy(c["x"]).double(), torch.from_numpy(c["a_replay"]).double(), N)
    q.retain_grad()
    t = torch.from_numpy(np.asarray(target_q, dtype=np.float64))
    w = torch.ones_like(t) if weights is None else torch.from_numpy(weights).double()
    loss = 0.5 * sum((w * (qc - t) ** 2).mean() for qc in q)
    loss.backward()
    n64 = lambda v: v.detach().double().numpy()      # noqa: E731
    return dict(loss=n64(loss), td_abs=n64((q - t).abs().mean(dim=0)), coef=n64(q.grad),
                grad={k: n64(p.grad) for k, p in P.items() if k.startswith("critic.")})


def actor_loss_ref(c, reduce, ent):
    """mean_r (ent logp - reduce_c q_c(x, a_pi)), reduce "min" or "mean": the loss, and the gradients of the actor's parameters and of x."""
    N = c["n_critics"]
    P = SC.as_torch(c["params"])
    x = torch.from_numpy(c["x"]).double().requires_grad_(True)
    act = SC.actor_forward(P, x, torch.from_numpy(c["noise_pi"]).double())
    q, _ = critic_forward(P, "critic", x, act["actions"], N)
    red = q.min(dim=0)[0] if reduce == "min" else q.mean(dim=0)
    loss = (ent * act["log_prob"] - red).mean()
    loss.backward()
    n64 = lambda v: v.detach().double().numpy()      # noqa: E731
    grad = {k: n64(p.grad) for k, p in P.items() if k.startswith("actor.")}
    grad["x"] = n64(x.grad)
    return dict(loss=n64(loss), grad=grad)


def polyak_ref(c):
    P = {k: np.asarray(v, dtype=np.float64) for k, v in c["params"].items()}
    return {k: (1 - c["tau"]) * v + c["tau"] * P["critic." + k[len("critic_target."):]] for k, v in P.items() if k.startswith("critic_target.")}
