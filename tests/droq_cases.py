"""Float64 restatement of the SAC DroQ critics (include/m3l_amd.h "SAC DroQ critics", m3l_amd/sac_ensemble.py with critic_layer_norm=True) and
the inputs of its tests (test_droq_cpu.py, test_droq_gpu.py, tools/sac_head_bench.py --droq), built on sac_ens_cases / sac_cases: the actor, the
batch, the inputs' scaling and the settle loop are theirs; the critics are N nets [Linear, Dropout, LayerNorm, ReLU] x n_qf + Linear(., 1).

The rule, from torch primitives (nn.functional.linear, explicit masks from test_dropout_cpu.dropout_mask, nn.functional.layer_norm, torch.relu,
autograd): z = W h + b;  d = z * mask * scale;  y = layer_norm(d) * gamma + beta (eps 1e-5);  h = relu(y).  The mask of hidden layer l of critic
c is dropout_mask(p, seed, c, l, B, w): c the critic's own index, also under a subset.  Neither SB3 nor a DroQ implementation is part of the
reference tree: PARITY UNPINNED.  With layer_norm=False and no masks `critic_forward` is sac_ens_cases.critic_forward, which test_droq_cpu.py
asserts.

`settle` nudges biases until, in float64, over every evaluation the tests make (all N critics at (x, a_replay) under the q seed's masks, without
masks (eval mode) and with the target critics' tensors; all N critics at (x, a_pi) under the q seed's masks; all N target critics at (x', a')
under the target seed's masks and without masks):
  * every post-LayerNorm y in front of a ReLU has |y| >= GATE_MARGIN (the LayerNorm's beta moves);
  * on every row the two smallest values among the target critics of every subset, with and without masks, and among all N critics at
    (x, a_pi), differ by at least TIE_MARGIN;
  * no pre-clamp log_std lies within CLAMP_MARGIN of an edge (the actor is sac_cases' and arrives settled; it is checked again)."""
from functools import lru_cache

import numpy as np
import torch
from torch.nn import functional as F

import sac_cases as SC
import sac_ens_cases as EC
from test_dropout_cpu import dropout_mask, keep_scale

ARCHS = dict(SC.ARCHS, w512=(64, (64,), (512,), 3))          # the LDS limit: eight 64-column groups

# name -> (arch, N, B, p): the smallest shapes at which each part can go wrong
CASES = {
    "aligned_n2_b1_p25": ("aligned", 2, 1, 0.25),          # w = 16: a LayerNorm over one MFMA tile, one row
    "mixed_n3_b33_p10": ("mixed", 3, 33, 0.1),             # widths 64 / 48 / 16: three sites, a width that is no multiple of 64, A = 1
    "a64_n2_b17_p01": ("a64", 2, 17, 0.01),                # the DroQ configuration: the anchor
    "a64_n2_b33_p0": ("a64", 2, 33, 0.0),                  # LayerNorm only
    "a64_n10_b33_p50": ("a64", 10, 33, 0.5),               # subset [9, 0]: the mask follows the critic's own index
    "amax_n3_b3_p10": ("amax", 3, 3, 0.1),                 # no hidden critic layer: no LayerNorm site
    "w512_n1_b17_p10": ("w512", 1, 17, 0.1),
}
ANCHOR = "a64_n2_b17_p01"
SEED_Q, SEED_T = 0x1F3D5B79A2C4E608, 0x0123456789ABCDEF          # the injected seeds of the q_values and td_target calls (63 bits)
EVALS = ("q_replay", "q_replay_eval", "q_replay_target", "q_pi", "q_next", "q_next_eval")


def critic_names(arch, N, prefix="critic"):
    """State-dict names of the N DroQ critics in creation order: per hidden layer the Linear at 4 l and the LayerNorm at 4 l + 2, then the output."""
    names, n = [], len(arch[2])
    for c in range(N):
        for l in range(n):
            names += [f"{prefix}.qf{c}.{4 * l + o}.{t}" for o in (0, 2) for t in ("weight", "bias")]
        names += [f"{prefix}.qf{c}.{4 * n}.weight", f"{prefix}.qf{c}.{4 * n}.bias"]
    return names


def param_names(arch, N):
    """Every name of the state dict of a SACEnsembleHead(critic_layer_norm=True), in creation order."""
    return SC.actor_names(arch) + critic_names(arch, N) + critic_names(arch, N, "critic_target")


def masks_of(c, seed):
    """{(critic, layer): bool tensor (B, w)} of a call with this seed, None when nothing drops (p = 0, or seed None: eval mode)."""
    p = c["dropout_p"]
    if seed is None or p <= 0.0:
        return None
    B = c["x"].shape[0]
    return {(ci, l): torch.from_numpy(dropout_mask(p, seed, ci, l, B, w)) for ci in range(c["n_critics"]) for l, w in enumerate(c["arch"][2])}


def critic_forward(P, prefix, x, actions, N, masks=None, scale=1.0, layer_norm=True):
    """N critics over cat([x.detach(), actions]) -> q (N, B) and, critic-major, what stands in front of every ReLU (y with LayerNorm, z without).
    masks: {(critic, layer): bool (B, w)} or None (all kept, scale 1)."""
    xa = torch.cat([x.detach(), actions], dim=1)
    step = 4 if layer_norm else 2
    qs, pres = [], []
    for c in range(N):
        h, l = xa, 0
        while f"{prefix}.qf{c}.{step * l + step}.weight" in P:
            z = F.linear(h, P[f"{prefix}.qf{c}.{step * l}.weight"], P[f"{prefix}.qf{c}.{step * l}.bias"])
            if layer_norm:
                if masks is not None:
                    z = z * masks[(c, l)].to(z.dtype) * scale
                z = F.layer_norm(z, (z.shape[1],), P[f"{prefix}.qf{c}.{4 * l + 2}.weight"], P[f"{prefix}.qf{c}.{4 * l + 2}.bias"], 1e-5)
            pres.append(z)
            h = torch.relu(z)
            l += 1
        qs.append(F.linear(h, P[f"{prefix}.qf{c}.{step * l}.weight"], P[f"{prefix}.qf{c}.{step * l}.bias"]).flatten())
    return torch.stack(qs), pres


def make_critics(arch, N, seed):
    """{name: float64 tensor}: N DroQ critics and their trailing targets: Linear outputs of standard deviation PRE_STD, gamma = 1 + 0.2 randn,
    beta = 0.2 randn, q of standard deviation 2, a target 0.9 critic + 0.1 fresh in every tensor."""
    Fd, _, qf, A = arch
    g = torch.Generator().manual_seed(seed)
    rn = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)      # noqa: E731
    xa = torch.cat([rn(512, Fd), torch.tanh(1.5 * rn(512, A))], dim=1)
    P = {}
    for prefix in ("critic", "critic_target"):
        for c in range(N):
            def put(key, v):
                P[f"{prefix}.qf{c}.{key}"] = v if prefix == "critic" else 0.9 * P[f"critic.qf{c}.{key}"] + 0.1 * v
                return P[f"{prefix}.qf{c}.{key}"]
            h = xa
            for l, w in enumerate(qf):
                W = rn(w, h.shape[1])
                W = put(f"{4 * l}.weight", W * (SC.PRE_STD / float(F.linear(h, W).std())))
                b = put(f"{4 * l}.bias", 0.2 * rn(w))
                gm, be = put(f"{4 * l + 2}.weight", 1.0 + 0.2 * rn(w)), put(f"{4 * l + 2}.bias", 0.2 * rn(w))
                h = torch.relu(F.layer_norm(F.linear(h, W, b), (w,), gm, be, 1e-5))
            W = rn(1, h.shape[1])
            put(f"{4 * len(qf)}.weight", W * (2.0 / float(F.linear(h, W).std())))
            put(f"{4 * len(qf)}.bias", 0.5 * rn(1))
    return P


def forward_ref(c, dtype=torch.float64):
    """Every forward value of the tests, without a tape -> float64 numpy: the actor's outputs at x and x', the six critic evaluations of EVALS,
    and the quantities of the input conditions (pre: owner-ordered as `_pre_owner`)."""
    P = SC.as_torch(c["params"], dtype)
    t = lambda k: torch.from_numpy(c[k]).to(dtype)      # noqa: E731
    N, sc = c["n_critics"], c["scale"]
    mq, mt = masks_of(c, SEED_Q), masks_of(c, SEED_T)
    n64 = lambda v: v.detach().double().numpy()      # noqa: E731
    out, pre = {}, []
    with torch.no_grad():
        act = SC.actor_forward(P, t("x"), t("noise_pi"), stable=dtype != torch.float64)
        nxt = SC.actor_forward(P, t("x_next"), t("noise_next"), stable=dtype != torch.float64)
        for name, prefix, x, a, masks in (("q_replay", "critic", "x", t("a_replay"), mq), ("q_replay_eval", "critic", "x", t("a_replay"), None),
                                          ("q_replay_target", "critic_target", "x", t("a_replay"), mq), ("q_pi", "critic", "x", act["actions"], mq),
                                          ("q_next", "critic_target", "x_next", nxt["actions"], mt), ("q_next_eval", "critic_target", "x_next", nxt["actions"], None)):
            q, ys = critic_forward(P, prefix, t(x), a, N, masks, sc)
            out[name] = n64(q)
            pre += ys
    out.update(a_pi=n64(act["actions"]), log_prob=n64(act["log_prob"]), a_next=n64(nxt["actions"]), log_prob_next=n64(nxt["log_prob"]),
               pre=[n64(p) for p in act["pre"] + nxt["pre"] + pre], s_pre=[n64(act["s_pre"]), n64(nxt["s_pre"])])
    return out


def _pre_owner(arch, N):
    """The bias behind each entry of forward_ref's `pre` list: the actor's Linear biases, then per evaluation the LayerNorm biases."""
    _, pi, qf, _ = arch
    actor = [f"actor.latent_pi.{2 * l}.bias" for l in range(len(pi))]
    crit = lambda prefix: [f"{prefix}.qf{c}.{4 * l + 2}.bias" for c in range(N) for l in range(len(qf))]      # noqa: E731
    return actor + actor + crit("critic") + crit("critic") + crit("critic_target") + crit("critic") + crit("critic_target") + crit("critic_target")


def tie_gaps(ref, N):
    """{what: smallest gap over the rows} for every minimum the tests take: each subset's target critics with and without masks, all N at (x, a_pi)."""
    out = {}
    for key in ("q_next", "q_next_eval"):
        for sub in EC.subsets(N):
            idx = sorted(set(range(N) if sub is None else sub))
            if len(idx) >= 2:
                out[f"{key} {sub}"] = float(EC.two_smallest_gap(ref[key][idx]).min())
    if N >= 2:
        out["q_pi"] = float(EC.two_smallest_gap(ref["q_pi"]).min())
    return out


def conditions(ref, N):
    pre = np.concatenate([p.ravel() for p in ref["pre"]]) if ref["pre"] else np.zeros(0)
    s = np.concatenate([p.ravel() for p in ref["s_pre"]])
    gaps = tie_gaps(ref, N)
    return dict(gate=float(np.abs(pre).min()) if pre.size else float("inf"), tie=min(gaps.values()) if gaps else float("inf"),
                clamp=float(np.minimum(np.abs(s - SC.LOG_STD_MIN), np.abs(s - SC.LOG_STD_MAX)).min()))


def settle(c, rounds=200):
    """sac_ens_cases.settle over this module's evaluations: the gate condition holds for the post-LayerNorm y and moves the LayerNorm's beta."""
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
        for prefix, q in (("critic_target", ref["q_next"]), ("critic_target", ref["q_next_eval"]), ("critic", ref["q_pi"])):
            for i in range(N):          # the later critic of a close pair moves
                for j in range(i + 1, N):
                    if (np.abs(q[i] - q[j]) < 1.5 * SC.TIE_MARGIN).any():
                        P[f"{prefix}.qf{j}.{4 * nq}.bias"] = (P[f"{prefix}.qf{j}.{4 * nq}.bias"] + 8 * SC.TIE_MARGIN).astype(np.float32)
                        moved = True
        if not moved:
            return c
    raise AssertionError("the input conditions did not settle")


def make_inputs(arch, N, B, p, seed):
    """sac_cases.make_inputs' batch and actor with N DroQ critics in place of its two, settled again.  float32 numpy arrays."""
    c = dict(SC.make_inputs(arch, B, False, True, seed))
    P = {k: v for k, v in c["params"].items() if k.startswith("actor.")}
    P.update({k: v.float().numpy() for k, v in make_critics(arch, N, seed + 2).items()})
    c["params"] = {k: P[k] for k in param_names(arch, N)}
    c.update(n_critics=N, dropout_p=p, scale=keep_scale(p) if p > 0 else 1.0)
    g = torch.Generator().manual_seed(seed + 3)
    c["weights"] = (0.25 + 1.5 * torch.rand(B, generator=g)).float().numpy()
    c["discounts"] = (SC.GAMMA ** (1 + torch.arange(B) % 3).double()).float().numpy()
    return settle(c)


@lru_cache(maxsize=None)
def case(name):
    arch, N, B, p = CASES[name]
    return make_inputs(ARCHS[arch], N, B, p, seed=6000 + 10 * sorted(CASES).index(name))


@lru_cache(maxsize=None)
def reference(name):
    return forward_ref(case(name))


def target_ref(c, ref, subset, gamma, ent, train=True):
    """sac_ens_cases.target_ref over the target critics under the target seed's masks (train) or without masks (eval mode)."""
    return EC.target_ref(c, dict(q_next=ref["q_next" if train else "q_next_eval"], log_prob_next=ref["log_prob_next"]), subset, gamma, ent)


def _n64(v):
    return v.detach().double().numpy()


def q_ref(c, actions, dq, prefix="critic", seed=SEED_Q, dtype=torch.float64):
    """q_values alone at (x, actions) under the masks of `seed` (None: eval mode) with a given output gradient (N, B): q, and the gradients in
    the actions and in W, b, gamma, beta of every critic and layer."""
    N = c["n_critics"]
    P = {k: v.detach().requires_grad_(True) for k, v in SC.as_torch(c["params"], dtype).items()}
    a = torch.from_numpy(actions).to(dtype).requires_grad_(True)
    x = torch.from_numpy(c["x"]).to(dtype).requires_grad_(True)
    q, _ = critic_forward(P, prefix, x, a, N, masks_of(c, seed), c["scale"])
    (q * torch.from_numpy(dq).to(dtype)).sum().backward()
    assert x.grad is None
    grad = {"actions": _n64(a.grad)}
    grad.update({k: _n64(p.grad) for k, p in P.items() if k.startswith(prefix + ".")})
    return dict(q=_n64(q), grad=grad)


def critic_loss_ref(c, target_q, weights=None, seed=SEED_Q, dtype=torch.float64):
    """sac_ens_cases.critic_loss_ref over the DroQ critics at (x, a_replay) under the masks of `seed`."""
    N = c["n_critics"]
    P = SC.as_torch(c["params"], dtype)
    q, _ = critic_forward(P, "critic", torch.from_numpy(c["x"]).to(dtype), torch.from_numpy(c["a_replay"]).to(dtype), N, masks_of(c, seed), c["scale"])
    t = torch.from_numpy(np.asarray(target_q, dtype=np.float64)).to(dtype)
    w = torch.ones_like(t) if weights is None else torch.from_numpy(weights).to(dtype)
    loss = 0.5 * sum((w * (qc - t) ** 2).mean() for qc in q)
    loss.backward()
    return dict(loss=_n64(loss), td_abs=_n64((q - t).abs().mean(dim=0)), grad={k: _n64(p.grad) for k, p in P.items() if k.startswith("critic.")})


def actor_loss_ref(c, reduce, ent, seed=SEED_Q, dtype=torch.float64):
    """sac_ens_cases.actor_loss_ref over the DroQ critics at (x, a_pi) under the masks of `seed`: the loss, the actor's gradients and x's."""
    N = c["n_critics"]
    P = SC.as_torch(c["params"], dtype)
    x = torch.from_numpy(c["x"]).to(dtype).requires_grad_(True)
    act = SC.actor_forward(P, x, torch.from_numpy(c["noise_pi"]).to(dtype), stable=dtype != torch.float64)
    q, _ = critic_forward(P, "critic", x, act["actions"], N, masks_of(c, seed), c["scale"])
    red = q.min(dim=0)[0] if reduce == "min" else q.mean(dim=0)
    loss = (ent * act["log_prob"] - red).mean()
    loss.backward()
    grad = {k: _n64(p.grad) for k, p in P.items() if k.startswith("actor.")}
    grad["x"] = _n64(x.grad)
    return dict(loss=_n64(loss), grad=grad)
