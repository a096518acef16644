"""Float64 restatement of the TD3 head (include/m3l_amd.h "TD3 head", m3l_amd/td3.py) and the inputs of its tests (test_td3_cpu.py,
test_td3_gpu.py, tools/sac_head_bench.py --td3), built on sac_ens_cases: the critics, their recipe and the margins are its; the deterministic
actor and its target are made here by the same recipe.

The rule, from torch primitives (nn.functional.linear, torch.relu, torch.tanh, torch.clamp, autograd): mu(x) = tanh(Linear_A(ReLU-MLP(x)));
smooth(a, n, sigma, c) = clamp(a + clamp(sigma n, -c, c), -1, 1) with both clamps passing the gradient straight through (DrQ-v2's
TruncatedNormal.sample(clip=)); the TD target's minimum over all N target critics at the smoothed action of the target (or the online) actor;
SB3's TD3 critic loss sum_c mean_r w_r (q_c - t)^2; the actor loss -mean_r reduce_c q_c with "first", "min" or "mean".  Neither SB3 nor a
DrQ-v2 implementation is part of the reference tree: PARITY UNPINNED.

Every case is evaluated in the three noise modes of MODES.  `settle` nudges biases and noise entries until, in float64, over every evaluation
the tests make (the actor at x and x', the target actor at x', all N critics at (x, a_replay) and at (x, actions) of every mode, all N target
critics at (x', a') of every mode and of either actor):
  * every ReLU pre-activation has |pre| >= GATE_MARGIN;
  * on every row the two smallest critics at (x, actions) differ by at least TIE_MARGIN, in every mode ("min" takes a gradient there);
  * no sigma n lies within CLAMP_MARGIN of +-c and no a + noise within CLAMP_MARGIN of +-1;
and the builder plants, in every noise tensor, one entry with |sigma n| > c whose action leaves [-1, 1] and one with |sigma n| < c."""
from functools import lru_cache

import numpy as np
import torch
from torch.nn import functional as F

import sac_cases as SC
import sac_ens_cases as EC

GATE_MARGIN, TIE_MARGIN, CLAMP_MARGIN = SC.GATE_MARGIN, SC.TIE_MARGIN, SC.CLAMP_MARGIN
SIGMA, CLIP = 0.6, 0.5          # a third of the standard-normal draws lie beyond c / sigma
MODES = {"det": (0.0, None), "clip": (SIGMA, CLIP), "noclip": (SIGMA, None)}
NOISY = ("clip", "noclip")

# (features, pi widths, qf widths, actions)
ARCHS = {k: SC.ARCHS[k] for k in ("a64", "mixed", "nohid", "amax")}
ARCHS["f16a7"] = (16, (32, 16), (32,), 7)          # F = 16, A = 7: F + A = 23

# name -> (arch, N, B)
CASES = {
    "a64_n2_b33": ("a64", 2, 33),            # the anchor: three row tiles, the last ragged
    "a64_n1_b17": ("a64", 1, 17),            # DDPG
    "a64_n3_b3": ("a64", 3, 3),
    "mixed_n3_b33": ("mixed", 3, 33),        # A = 1; one hidden actor layer, three per critic
    "nohid_n10_b3": ("nohid", 10, 3),        # an actor without a hidden layer; the most critics
    "amax_n2_b17": ("amax", 2, 17),          # A = 64; critics without a hidden layer
    "amax_n3_b1": ("amax", 3, 1),            # one row
    "f16a7_n2_b17": ("f16a7", 2, 17),        # A = 7, F = 16
    "f16a7_n10_b1": ("f16a7", 10, 1),
}
ANCHOR = "a64_n2_b33"
# which noise tensor goes with which evaluation of an actor
EVALS = {"pi": ("actor", "x", "noise_pi"), "next": ("actor_target", "x_next", "noise_next"), "next_online": ("actor", "x_next", "noise_next_online")}


def actor_names(arch, prefix="actor"):
    """State-dict names of an actor in TD3Params.actor_flat order."""
    return [f"{prefix}.mu.{2 * l}.{t}" for l in range(len(arch[1]) + 1) for t in ("weight", "bias")]


def param_names(arch, N):
    """Every name of a TD3Head's state dict, in creation order (SB3's TD3Policy: actor, actor_target, critic, critic_target)."""
    return actor_names(arch) + actor_names(arch, "actor_target") + EC.critic_names(arch, N) + EC.critic_names(arch, N, "critic_target")


def actor_forward(P, prefix, x):
    """SB3's td3 Actor after extract_features: mu = tanh(Linear_A(ReLU-MLP(x))) -> (mu, the head's pre-activation, the ReLU pre-activations)."""
    h, pres, l = x, [], 0
    while f"{prefix}.mu.{2 * l + 2}.weight" in P:
        pre = F.linear(h, P[f"{prefix}.mu.{2 * l}.weight"], P[f"{prefix}.mu.{2 * l}.bias"])
        pres.append(pre)
        h = torch.relu(pre)
        l += 1
    u = F.linear(h, P[f"{prefix}.mu.{2 * l}.weight"], P[f"{prefix}.mu.{2 * l}.bias"])
    return torch.tanh(u), u, pres


def smooth(a, noise, sigma, clip):
    """clamp(a + clamp(sigma noise, -c, c), -1, 1); the outer clamp passes the gradient straight through; sigma = 0: a itself."""
    if sigma == 0.0:
        return a
    e = sigma * noise
    if clip is not None:
        e = torch.clamp(e, -clip, clip)
    v = a + e
    return v - v.detach() + torch.clamp(v, -1.0, 1.0).detach()


def make_actor(arch, seed):
    """{name: float64 tensor}: a trained-like actor (hidden pre-activations of standard deviation PRE_STD, the head's of 1.3, so |mu| reaches
    0.99) and a target that trails it (0.9 actor + 0.1 fresh)."""
    Fd, pi, _, A = arch
    g = torch.Generator().manual_seed(seed)
    rn = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)      # noqa: E731
    x = rn(512, Fd)
    P = {}
    for prefix in ("actor", "actor_target"):
        h = x
        for l, w in enumerate(tuple(pi) + (A,)):
            last = l == len(pi)
            W, b = rn(w, h.shape[1]), (0.1 if last else 0.2) * rn(w)
            W = W * ((1.3 if last else SC.PRE_STD) / float(F.linear(h, W).std()))
            if prefix == "actor_target":
                W = 0.9 * P[f"actor.mu.{2 * l}.weight"] + 0.1 * W
                b = 0.9 * P[f"actor.mu.{2 * l}.bias"] + 0.1 * b
            P[f"{prefix}.mu.{2 * l}.weight"], P[f"{prefix}.mu.{2 * l}.bias"] = W, b
            h = torch.relu(F.linear(h, W, b))
    return P


def as_torch(P, dtype=torch.float64):
    """Leaves that take a gradient, except both target nets."""
    return {k: torch.from_numpy(np.asarray(v)).to(dtype).requires_grad_("_target." not in k) for k, v in P.items()}


def forward_ref(c):
    """Every forward value the tests compare, without a tape -> float64 numpy.  mu: the three actor evaluations of EVALS; per mode: actions
    (`pi`), a' of the target actor (`next`) and of the online one (`next_online`), q of the critics there; q_replay; gates: (bias name,
    pre-activation) of every ReLU evaluated."""
    P = as_torch(c["params"])
    N = c["n_critics"]
    t = lambda k: torch.from_numpy(c[k]).double()      # noqa: E731
    n64 = lambda v: v.detach().double().numpy()      # noqa: E731
    out = dict(mu={}, a={m: {} for m in MODES}, q={m: {} for m in MODES}, gates=[])
    crit_owner = lambda prefix: [f"{prefix}.qf{i}.{2 * l}.bias" for i in range(N) for l in range(len(c["arch"][2]))]      # noqa: E731
    with torch.no_grad():
        for ev, (prefix, xk, nk) in EVALS.items():
            mu, _, pres = actor_forward(P, prefix, t(xk))
            out["mu"][ev] = n64(mu)
            out["gates"] += [(f"{prefix}.mu.{2 * l}.bias", n64(p)) for l, p in enumerate(pres)]
            cp = "critic" if ev == "pi" else "critic_target"
            for m, (sigma, clip) in MODES.items():
                a = smooth(mu, t(nk), sigma, clip)
                q, pres_q = EC.critic_forward(P, cp, t(xk), a, N)
                out["a"][m][ev], out["q"][m][ev] = n64(a), n64(q)
                out["gates"] += list(zip(crit_owner(cp), [n64(p) for p in pres_q]))
        q, pres_q = EC.critic_forward(P, "critic", t("x"), t("a_replay"), N)
        out["q_replay"] = n64(q)
        out["gates"] += list(zip(crit_owner("critic"), [n64(p) for p in pres_q]))
    return out


def clamp_distances(c, ref):
    """{(evaluation, mode): (distance of |sigma n| from c, distance of |a + noise| from 1)} as arrays (B, A), float64; inf where no clamp is."""
    out = {}
    for ev, (_, _, nk) in EVALS.items():
        for m in NOISY:
            sigma, clip = MODES[m]
            e = sigma * c[nk].astype(np.float64)
            inner = np.abs(np.abs(e) - clip) if clip is not None else np.full(e.shape, np.inf)
            v = ref["mu"][ev] + (np.clip(e, -clip, clip) if clip is not None else e)
            out[ev, m] = (inner, np.abs(np.abs(v) - 1.0), e, v)
    return out


def conditions(c, ref):
    """The distances the comparisons rest on, and how many entries lie on the far side of each clamp."""
    N = c["n_critics"]
    pre = np.concatenate([p.ravel() for _, p in ref["gates"]]) if ref["gates"] else np.zeros(0)
    tie = min([float(EC.two_smallest_gap(ref["q"][m]["pi"]).min()) for m in MODES] if N >= 2 else [float("inf")])
    dist = clamp_distances(c, ref)
    sides = {}
    for (ev, m), (inner, outer, e, v) in dist.items():
        clip = MODES[m][1]
        sides[ev, m] = dict(inner_out=int((np.abs(e) > clip).sum()) if clip is not None else None,
                            inner_in=int((np.abs(e) < clip).sum()) if clip is not None else None, outer_out=int((np.abs(v) > 1.0).sum()))
    return dict(gate=float(np.abs(pre).min()) if pre.size else float("inf"), tie=tie,
                clamp=float(min(min(inner.min(), outer.min()) for inner, outer, _, _ in dist.values())), sides=sides)


def plant(c):
    """In every noise tensor: the entry whose deterministic action is largest takes sigma n = 2 c towards the nearer edge (clipped to c it still
    leaves [-1, 1]), another entry takes sigma n = c / 4."""
    ref = forward_ref(c)
    for ev, (_, _, nk) in EVALS.items():
        mu = ref["mu"][ev].ravel()
        assert mu.size >= 2, "a noisy case needs at least two action entries"
        k = int(np.abs(mu).argmax())
        assert abs(mu[k]) > 1.0 - CLIP + 0.05, f"{nk}: no action beyond {1.0 - CLIP}"
        flat = c[nk].reshape(-1)
        flat[k] = np.float32(np.sign(mu[k]) * 2.0 * CLIP / SIGMA)
        flat[(k + 1) % mu.size] = np.float32(0.25 * CLIP / SIGMA)


def settle(c, rounds=200):
    """Nudge biases and noise entries (by a few margins at a time, in float32 steps) until the input conditions of the module docstring hold."""
    N, nq = c["n_critics"], len(c["arch"][2])
    P = c["params"]
    for _ in range(rounds):
        ref = forward_ref(c)
        moved = False
        for name, pre in ref["gates"]:
            bad = (np.abs(pre) < 1.5 * GATE_MARGIN).any(axis=0)
            if bad.any():
                P[name] = (P[name] + np.where(bad, 4 * GATE_MARGIN, 0.0)).astype(np.float32)
                moved = True
        for m in MODES:
            q = ref["q"][m]["pi"]
            for i in range(N):          # the later critic of a close pair moves
                for j in range(i + 1, N):
                    if (np.abs(q[i] - q[j]) < 1.5 * TIE_MARGIN).any():
                        P[f"critic.qf{j}.{2 * nq}.bias"] = (P[f"critic.qf{j}.{2 * nq}.bias"] + 8 * TIE_MARGIN).astype(np.float32)
                        moved = True
        for (ev, m), (inner, outer, e, _) in clamp_distances(c, ref).items():
            nk, clip = EVALS[ev][2], MODES[m][1]
            near_in, near_out = inner < 1.5 * CLAMP_MARGIN, outer < 1.5 * CLAMP_MARGIN
            if near_in.any() or near_out.any():
                n = c[nk].astype(np.float64)
                step = np.where(n >= 0, 1.0, -1.0) * 4 * CLAMP_MARGIN / SIGMA
                held = near_out & (np.abs(e) > clip) if clip is not None else np.zeros_like(near_out)      # clipped: moving n moves nothing
                n = np.where(held, np.where(n >= 0, 1.0, -1.0) * 0.37 * CLIP / SIGMA, np.where(near_in | near_out, n + step, n))
                c[nk] = n.astype(np.float32)
                moved = True
        if not moved:
            return c
    raise AssertionError("the input conditions did not settle")


def check(c):
    """The input conditions, asserted: what the builder guarantees and test_td3_cpu.py asserts again."""
    cond = conditions(c, forward_ref(c))
    assert cond["gate"] >= GATE_MARGIN and cond["tie"] >= TIE_MARGIN and cond["clamp"] >= CLAMP_MARGIN, cond
    for key, s in cond["sides"].items():
        assert s["outer_out"] >= 1 and (s["inner_out"] is None or (s["inner_out"] >= 1 and s["inner_in"] >= 1)), (key, s)
    return cond


def make_inputs(arch, N, B, seed):
    """One replay batch for a head: parameters, features of both observations, one noise draw per actor evaluation, replay actions, rewards,
    dones (both 0 and 1 when B > 1), importance weights, n-step discounts and the step's constants.  float32 numpy arrays, planted and settled."""
    Fd, _, _, A = arch
    P = {k: v.float().numpy() for k, v in make_actor(arch, seed).items()}
    P.update({k: v.float().numpy() for k, v in EC.make_critics(arch, N, seed + 2).items()})
    g = torch.Generator().manual_seed(seed + 1)
    rn = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64).float().numpy()      # noqa: E731
    dones = (torch.rand(B, generator=g) < 0.3).float().numpy()
    if B > 1:
        dones[0], dones[1] = 0.0, 1.0
    c = dict(params={k: P[k] for k in param_names(arch, N)}, x=rn(B, Fd), x_next=rn(B, Fd), noise_pi=rn(B, A), noise_next=rn(B, A),
             noise_next_online=rn(B, A), a_replay=np.tanh(1.5 * rn(B, A)).astype(np.float32), rewards=rn(B), dones=dones, gamma=SC.GAMMA, tau=SC.TAU,
             arch=arch, n_critics=N)
    c["weights"] = (0.25 + 1.5 * torch.rand(B, generator=g)).float().numpy()
    c["discounts"] = (SC.GAMMA ** (1 + torch.arange(B) % 3).double()).float().numpy()
    plant(c)
    settle(c)
    check(c)
    return c


@lru_cache(maxsize=None)
def case(name):
    arch, N, B = CASES[name]
    return make_inputs(ARCHS[arch], N, B, seed=6000 + 10 * sorted(CASES).index(name))


@lru_cache(maxsize=None)
def reference(name):
    return forward_ref(case(name))


def _n64(v):
    return v.detach().double().numpy()


def actions_ref(c, mode, dactions, ev="pi"):
    """`actions` alone for one evaluation of EVALS with a given output gradient: the actions, and the gradients in the features and in that
    actor's parameters (as if the target took one, so that every actor evaluation can be checked)."""
    prefix, xk, nk = EVALS[ev]
    P = {k: v.detach().requires_grad_(True) for k, v in as_torch(c["params"]).items()}
    x = torch.from_numpy(c[xk]).double().requires_grad_(True)
    mu, _, _ = actor_forward(P, prefix, x)
    a = smooth(mu, torch.from_numpy(c[nk]).double(), *MODES[mode])
    (a * torch.from_numpy(dactions).double()).sum().backward()
    grad = {"x": _n64(x.grad)}
    grad.update({k: _n64(p.grad) for k, p in P.items() if k.startswith(prefix + ".")})
    return dict(actions=_n64(a), grad=grad)


def target_ref(c, ref, mode, gamma, online=False):
    """target_q (B,) in float64: r + (1 - done) g min_c q_target_c(x', a'); gamma a number or (B,)."""
    nq = ref["q"][mode]["next_online" if online else "next"].min(axis=0)
    return c["rewards"].astype(np.float64) + (1.0 - c["dones"].astype(np.float64)) * np.asarray(gamma, dtype=np.float64) * nq


def critic_loss_ref(c, target_q, weights=None):
    """SB3's TD3 critic loss at (x, a_replay) against a given target: loss = sum_c mean_r w_r (q_c - t)^2, td_abs = mean_c |q_c - t|, coef =
    d loss / d q, and the gradient of every critic parameter."""
    N = c["n_critics"]
    P = as_torch(c["params"])
    q, _ = EC.critic_forward(P, "critic", torch.from_numpy(c["x"]).double(), torch.from_numpy(c["a_replay"]).double(), N)
    q.retain_grad()
    t = torch.from_numpy(np.asarray(target_q, dtype=np.float64))
    w = torch.ones_like(t) if weights is None else torch.from_numpy(weights).double()
    loss = sum((w * (qc - t) ** 2).mean() for qc in q)
    loss.backward()
    return dict(loss=_n64(loss), td_abs=_n64((q - t).abs().mean(dim=0)), coef=_n64(q.grad),
                grad={k: _n64(p.grad) for k, p in P.items() if k.startswith("critic.")})


def actor_loss_ref(c, reduce, mode="det"):
    """-mean_r reduce_c q_c(x, actions), reduce "first", "min" or "mean": the loss, and the gradients of the actor's parameters and of x."""
    N = c["n_critics"]
    P = as_torch(c["params"])
    x = torch.from_numpy(c["x"]).double().requires_grad_(True)
    mu, _, _ = actor_forward(P, "actor", x)
    a = smooth(mu, torch.from_numpy(c["noise_pi"]).double(), *MODES[mode])
    q, _ = EC.critic_forward(P, "critic", x, a, N)
    red = {"first": lambda: q[0], "min": lambda: q.min(dim=0)[0], "mean": lambda: q.mean(dim=0)}[reduce]()
    loss = -red.mean()
    loss.backward()
    grad = {k: _n64(p.grad) for k, p in P.items() if k.startswith("actor.")}
    grad["x"] = _n64(x.grad)
    return dict(loss=_n64(loss), grad=grad)


def polyak_ref(c):
    P = {k: np.asarray(v, dtype=np.float64) for k, v in c["params"].items()}
    return {k: (1 - c["tau"]) * v + c["tau"] * P[k.replace("_target.", ".", 1)] for k, v in P.items() if "_target." in k}


def step_ref(c, mode="clip", reduce="first"):
    """The head's part of one TD3 gradient step, in order: the target (target actor, smoothed in `mode`), the critic loss and its backward, the
    actor loss (deterministic actions, `reduce`) and its backward, the Polyak update of both target nets."""
    ref = forward_ref(c)
    target_q = target_ref(c, ref, mode, c["gamma"])
    cl = critic_loss_ref(c, target_q)
    al = actor_loss_ref(c, reduce)
    grad = dict(cl["grad"])
    grad.update(al["grad"])
    return dict(target_q=target_q, critic_loss=cl["loss"], actor_loss=al["loss"], grad=grad, target=polyak_ref(c))
