"""Time of the SAC policy head on synthetic features (EXPERIMENTS.md "SAC policy head"); no simulator, no extractor.  The sibling of
policy_head_bench.py, with its method (alternating windows, device events, the library's event brackets, torch.profiler's kernel records).

  (a) the head's part of one gradient step of SAC_MAE.train (sac_mae.py:303-366) at B = 256, F = 256, pi = qf = [256, 256], A = 7,
      ent_coef = "auto" (Train_sacmae.py): action_log_prob, the entropy-coefficient loss and its backward, the TD target, the critic loss and
      its backward, the actor loss and its backward, the Polyak update.  Optimizer steps are not part of it on either path.
  (b) the actor under no_grad at B = 8: the head of one environment step

each on two paths on the same GPU:
  hip    m3l_amd.SACHead (m3l_amd/csrc/sac.hip)
  eager  the float32 torch restatement of the same arithmetic (tests/sac_cases.py: nn.functional.linear, relu, clamp, tanh,
         torch.distributions.Normal, the lines of sac_mae.py, autograd, SB3's polyak_update loop): what a user of the reference runs today
and, for (a), with and without the reads of the logged values: the reference reads four scalars one by one (`.item()`, sac_mae.py:313, 317, 344,
357), the HIP path needs none for the step and reads its four 0-d tensors in one stacked copy when they are to be logged.

The figures per path are policy_head_bench.py's (call_us, host_us, entry_points, kernel_us / launches / copies).  Both paths' losses are printed,
so that a wrong result cannot pass as a fast one.  Without a GPU the tool fails; it has no fallback.

With --critics N the tool measures the critic ensemble instead (EXPERIMENTS.md "SAC critic ensemble"), at the same shapes: per call of
`q_values` forward + backward, of `td_target` over a subset of M (--subset, default 2) and of a whole critic update (target, loss, backward,
Polyak update), and of one actor update with --q-reduce, on
  ens    m3l_amd.SACEnsembleHead with N critics
  eager  the float32 torch restatement looping over the N critics (tests/sac_ens_cases.py)
  twin   m3l_amd.SACHead on the same two critics, when N = 2 (the subset is then None: both)
in alternating windows of one run.

With --droq it measures one critic update (TD target, critic loss, backward, Polyak update) of the DroQ critics (EXPERIMENTS.md "SAC DroQ
critics") at N = 2, the same shapes, p = 0.01, on
  droq   m3l_amd.SACEnsembleHead(n_critics=2, critic_layer_norm=True, critic_dropout=0.01)
  eager  the float32 torch restatement of tests/droq_cases.py with torch's own dropout in place of the contract's masks
  ens10  the existing update of m3l_amd.SACEnsembleHead with N = 10 critics and a subset of 2, the REDQ recipe DroQ stands in for
in alternating windows of one run.

With --tqc it measures one critic update of the TQC head (EXPERIMENTS.md "SAC TQC critics"): `td_target` + `critic_loss` + backward at the same
shapes, n_quantiles = 25, top_quantiles_to_drop_per_net = 2 and N = 2 critics (--critics N for another count, e.g. 10), on
  tqc    m3l_amd.TQCHead
  eager  the float32 torch restatement of tests/tqc_cases.py (torch.sort over the pooled quantiles, the 4-D broadcast of the quantile-Huber loss)
  ens2   the same three calls of m3l_amd.SACEnsembleHead with N = 2 critics, the scalar-critic update TQC replaces
in alternating windows of one run.

With --td3 it measures the TD3 head (EXPERIMENTS.md "TD3 head") at the same shapes and N = 2: a critic update (`td_target` with SB3's target-policy
smoothing, `critic_loss`, backward) and an actor update (`actor_loss` with q_reduce="first", backward), on
  td3    m3l_amd.TD3Head
  eager  the float32 torch restatement of tests/td3_cases.py
  ens2   the same calls of m3l_amd.SACEnsembleHead with N = 2 critics (its actor loss with the min reduction), the stochastic head's update
in alternating windows of one run.

Usage: python tools/sac_head_bench.py [--iters 500] [--rounds 5] [--warmup 30] [--critics N [--subset M] [--q-reduce min|mean] | --droq | --tqc [--critics N] | --td3]
(one JSON line on stdout)"""
import argparse
import json
import os
import sys

import torch
from torch.nn import functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import sac_cases as SC  # noqa: E402
import sac_ens_cases as EC  # noqa: E402
import droq_cases as DC  # noqa: E402
import tqc_cases as TC  # noqa: E402
import td3_cases as T3C  # noqa: E402
import m3l_amd  # noqa: E402
from m3l_amd import sac as SH  # noqa: E402
from policy_head_bench import alternate, counted, entry_points  # noqa: E402

DEV = "cuda:0"
ARCH = (256, (256, 256), (256, 256), 7)


def ensemble(a):
    """The --critics mode: see the module docstring."""
    N, M = a.critics, None if a.critics == 2 else min(a.subset, a.critics)
    c = EC.make_inputs(ARCH, N, 256, seed=9)
    head = m3l_amd.SACEnsembleHead(ARCH[0], ARCH[3], net_arch=dict(pi=list(ARCH[1]), qf=list(ARCH[2])), n_critics=N)
    head.load_state_dict({k: torch.from_numpy(v) for k, v in c["params"].items()})
    head = head.to(DEV)
    heads = {"ens": head}
    if N == 2:
        heads["twin"] = m3l_amd.SACHead(ARCH[0], ARCH[3], net_arch=dict(pi=list(ARCH[1]), qf=list(ARCH[2]))).to(DEV)
        heads["twin"].load_state_dict(head.state_dict())
    P = dict(head.named_parameters())
    t = {k: torch.from_numpy(c[k]).to(DEV) for k in ("x", "x_next", "noise_pi", "noise_next", "a_replay", "rewards", "dones")}
    log_ent = torch.tensor([c["log_ent_coef"]], dtype=torch.float32, device=DEV)
    critic_params = [p for n, p in P.items() if n.startswith("critic.")]
    target_params = [p for n, p in P.items() if n.startswith("critic_target.")]
    gamma, tau = c["gamma"], c["tau"]
    subset = None if M is None else torch.arange(M, dtype=torch.int32, device=DEV)
    dq = torch.ones(N, 256, device=DEV)

    def zero(h):
        for p in h.parameters():
            p.grad = None

    def hip_target(h):
        kw = {} if h is not head else dict(subset=head.sample_subset(M) if M else None)
        return h.td_target(t["x_next"], t["rewards"], t["dones"], gamma, log_ent_coef=log_ent, noise=t["noise_next"], **kw)

    def eager_target():
        with torch.no_grad():
            n = SC.actor_forward(P, t["x_next"], t["noise_next"])
            idx = torch.randperm(N, device=DEV)[:M] if M else torch.arange(N, device=DEV)
            qn, _ = EC.critic_forward(P, "critic_target", t["x_next"], n["actions"], N)      # SB3's critic evaluates all N; the subset picks rows
            nq = qn[idx].min(dim=0)[0] - torch.exp(log_ent) * n["log_prob"]
            return t["rewards"] + (1 - t["dones"]) * gamma * nq

    def hip_q(h):
        zero(h)
        q = h.q_values(t["x"], t["a_replay"])
        q.backward(dq)
        return q

    def eager_q():
        zero(head)
        q, _ = EC.critic_forward(P, "critic", t["x"], t["a_replay"], N)
        q.backward(dq)
        return q

    def hip_update(h):
        zero(h)
        loss = h.critic_loss(t["x"], t["a_replay"], hip_target(h))
        loss.backward()
        h.polyak_update(tau)
        return loss

    def eager_update():
        zero(head)
        target_q = eager_target()
        q, _ = EC.critic_forward(P, "critic", t["x"], t["a_replay"], N)
        loss = 0.5 * sum(F.mse_loss(qc, target_q) for qc in q)
        loss.backward()
        with torch.no_grad():
            for p, tp in zip(critic_params, target_params):
                tp.mul_(1 - tau)
                torch.add(tp, p, alpha=tau, out=tp)
        return loss

    def hip_actor(h):
        zero(h)
        kw = dict(q_reduce=a.q_reduce) if h is head else {}
        loss, _ = h.actor_loss(t["x"], log_ent_coef=log_ent, noise=t["noise_pi"], **kw)
        loss.backward()
        return loss

    def eager_actor():
        zero(head)
        o = SC.actor_forward(P, t["x"], t["noise_pi"])
        q, _ = EC.critic_forward(P, "critic", t["x"], o["actions"], N)
        red = q.min(dim=0)[0] if a.q_reduce == "min" else q.mean(dim=0)
        loss = (torch.exp(log_ent) * o["log_prob"] - red).mean()
        loss.backward()
        return loss
    out = {"arch": {"features": ARCH[0], "pi": list(ARCH[1]), "qf": list(ARCH[2]), "actions": ARCH[3]}, "critics": N, "subset": M,
           "q_reduce": a.q_reduce, "B": 256}          # SACHead's actor loss is the min: compare N = 2 with --q-reduce min
    for what, hip_fn, eager_fn in (("q_values_fwd_bwd", hip_q, eager_q), ("td_target", hip_target, eager_target), ("critic_update", hip_update, eager_update),
                                   ("actor_update", hip_actor, eager_actor)):
        fns = {name: (lambda h=h, f=hip_fn: f(h)) for name, h in heads.items()}
        fns["eager"] = eager_fn
        res, last = alternate(fns, a.iters, a.warmup, a.rounds)
        for name, fn in fns.items():
            res[name].update(counted(fn))
            res[name]["result_sum"] = float(last[name].detach().float().sum())
        res["ens"]["entry_points"] = entry_points(fns["ens"])
        res["ens_over_eager_call"] = round(res["ens"]["call_us"] / res["eager"]["call_us"], 3)
        if "twin" in res:
            res["ens_over_twin_call"] = round(res["ens"]["call_us"] / res["twin"]["call_us"], 3)
        out[what] = res
    print(json.dumps(out))


def droq(a):
    """The --droq mode: see the module docstring."""
    N, B, p = 2, 256, 0.01
    c = DC.make_inputs(ARCH, N, B, p, seed=9)
    net_arch = dict(pi=list(ARCH[1]), qf=list(ARCH[2]))
    head = m3l_amd.SACEnsembleHead(ARCH[0], ARCH[3], net_arch=net_arch, n_critics=N, critic_layer_norm=True, critic_dropout=p)
    head.load_state_dict({k: torch.from_numpy(v) for k, v in c["params"].items()})
    head = head.to(DEV)
    ce = EC.make_inputs(ARCH, 10, B, seed=9)
    ens = m3l_amd.SACEnsembleHead(ARCH[0], ARCH[3], net_arch=net_arch, n_critics=10)
    ens.load_state_dict({k: torch.from_numpy(v) for k, v in ce["params"].items()})
    ens = ens.to(DEV)
    P = dict(head.named_parameters())
    t = {k: torch.from_numpy(c[k]).to(DEV) for k in ("x", "x_next", "noise_pi", "noise_next", "a_replay", "rewards", "dones")}
    log_ent = torch.tensor([c["log_ent_coef"]], dtype=torch.float32, device=DEV)
    critic_params = [q for n, q in P.items() if n.startswith("critic.")]
    target_params = [q for n, q in P.items() if n.startswith("critic_target.")]
    gamma, tau = c["gamma"], c["tau"]

    def zero(h):
        for q in h.parameters():
            q.grad = None

    def eager_critics(prefix, x, actions):
        """The restatement's critics in float32 with torch's own dropout in place of the contract's masks (other masks, the same work)."""
        xa = torch.cat([x, actions], dim=1)
        qs = []
        for ci in range(N):
            h = xa
            for l, w in enumerate(ARCH[2]):
                z = F.dropout(F.linear(h, P[f"{prefix}.qf{ci}.{4 * l}.weight"], P[f"{prefix}.qf{ci}.{4 * l}.bias"]), p, True)
                h = torch.relu(F.layer_norm(z, (w,), P[f"{prefix}.qf{ci}.{4 * l + 2}.weight"], P[f"{prefix}.qf{ci}.{4 * l + 2}.bias"], 1e-5))
            qs.append(F.linear(h, P[f"{prefix}.qf{ci}.{4 * len(ARCH[2])}.weight"], P[f"{prefix}.qf{ci}.{4 * len(ARCH[2])}.bias"]).flatten())
        return torch.stack(qs)

    def hip_update(h, **kw):
        zero(h)
        target_q = h.td_target(t["x_next"], t["rewards"], t["dones"], gamma, log_ent_coef=log_ent, noise=t["noise_next"], **kw)
        loss = h.critic_loss(t["x"], t["a_replay"], target_q)
        loss.backward()
        h.polyak_update(tau)
        return loss

    def eager_update():
        zero(head)
        with torch.no_grad():
            n = SC.actor_forward(P, t["x_next"], t["noise_next"])
            nq = eager_critics("critic_target", t["x_next"], n["actions"]).min(dim=0)[0] - torch.exp(log_ent) * n["log_prob"]
            target_q = t["rewards"] + (1 - t["dones"]) * gamma * nq
        q = eager_critics("critic", t["x"], t["a_replay"])
        loss = 0.5 * sum(F.mse_loss(qc, target_q) for qc in q)
        loss.backward()
        with torch.no_grad():
            for q_, tp in zip(critic_params, target_params):
                tp.mul_(1 - tau)
                torch.add(tp, q_, alpha=tau, out=tp)
        return loss
    fns = {"droq": lambda: hip_update(head), "eager": eager_update, "ens10": lambda: hip_update(ens, subset=ens.sample_subset(2))}
    res, last = alternate(fns, a.iters, a.warmup, a.rounds)
    for name, fn in fns.items():
        res[name].update(counted(fn))
        res[name]["result_sum"] = float(last[name].detach().float().sum())
    res["droq"]["entry_points"] = entry_points(fns["droq"])
    res["droq_over_eager_call"] = round(res["droq"]["call_us"] / res["eager"]["call_us"], 3)
    res["droq_over_ens10_call"] = round(res["droq"]["call_us"] / res["ens10"]["call_us"], 3)
    print(json.dumps({"arch": {"features": ARCH[0], "pi": list(ARCH[1]), "qf": list(ARCH[2]), "actions": ARCH[3]}, "critics": N, "dropout": p, "B": B,
                      "critic_update": res}))


def tqc(a):
    """The --tqc mode: see the module docstring."""
    N, nq, drop, B = a.critics or 2, 25, 2, 256
    c = TC.make_inputs(ARCH, N, nq, drop, B, seed=9)
    K = c["K"]
    net_arch = dict(pi=list(ARCH[1]), qf=list(ARCH[2]))
    head = m3l_amd.TQCHead(ARCH[0], ARCH[3], net_arch=net_arch, n_critics=N, n_quantiles=nq, top_quantiles_to_drop_per_net=drop)
    head.load_state_dict({k: torch.from_numpy(v) for k, v in c["params"].items()})
    head = head.to(DEV)
    ce = EC.make_inputs(ARCH, 2, B, seed=9)
    ens = m3l_amd.SACEnsembleHead(ARCH[0], ARCH[3], net_arch=net_arch, n_critics=2)
    ens.load_state_dict({k: torch.from_numpy(v) for k, v in ce["params"].items()})
    ens = ens.to(DEV)
    P = dict(head.named_parameters())
    t = {k: torch.from_numpy(c[k]).to(DEV) for k in ("x", "x_next", "noise_pi", "noise_next", "a_replay", "rewards", "dones")}
    log_ent = torch.tensor([c["log_ent_coef"]], dtype=torch.float32, device=DEV)
    gamma = c["gamma"]

    def zero(h):
        for q in h.parameters():
            q.grad = None

    def hip_update(h):
        zero(h)
        target = h.td_target(t["x_next"], t["rewards"], t["dones"], gamma, log_ent_coef=log_ent, noise=t["noise_next"])
        loss = h.critic_loss(t["x"], t["a_replay"], target)
        loss.backward()
        return loss

    def eager_update():
        zero(head)
        with torch.no_grad():
            n = SC.actor_forward(P, t["x_next"], t["noise_next"])
            zn, _ = TC.critic_forward(P, "critic_target", t["x_next"], n["actions"], N)
            target = TC.truncated_target(zn, n["log_prob"], t["rewards"], t["dones"], gamma, torch.exp(log_ent), K)
        z, _ = TC.critic_forward(P, "critic", t["x"], t["a_replay"], N)
        loss = TC.quantile_huber_loss(z, target)
        loss.backward()
        return loss
    fns = {"tqc": lambda: hip_update(head), "eager": eager_update, "ens2": lambda: hip_update(ens)}
    res, last = alternate(fns, a.iters, a.warmup, a.rounds)
    for name, fn in fns.items():
        res[name].update(counted(fn))
        res[name]["result_sum"] = float(last[name].detach().float().sum())
    res["tqc"]["entry_points"] = entry_points(fns["tqc"])
    res["tqc_over_eager_call"] = round(res["tqc"]["call_us"] / res["eager"]["call_us"], 3)
    res["tqc_over_ens2_call"] = round(res["tqc"]["call_us"] / res["ens2"]["call_us"], 3)
    print(json.dumps({"arch": {"features": ARCH[0], "pi": list(ARCH[1]), "qf": list(ARCH[2]), "actions": ARCH[3]}, "critics": N, "n_quantiles": nq,
                      "top_quantiles_to_drop_per_net": drop, "K": K, "B": B, "critic_update": res}))


def td3(a):
    """The --td3 mode: see the module docstring."""
    N, B = 2, 256
    c = T3C.make_inputs(ARCH, N, B, seed=9)
    net_arch = dict(pi=list(ARCH[1]), qf=list(ARCH[2]))
    head = m3l_amd.TD3Head(ARCH[0], ARCH[3], net_arch=net_arch, n_critics=N)
    head.load_state_dict({k: torch.from_numpy(v) for k, v in c["params"].items()})
    head = head.to(DEV)
    ce = EC.make_inputs(ARCH, N, B, seed=9)
    ens = m3l_amd.SACEnsembleHead(ARCH[0], ARCH[3], net_arch=net_arch, n_critics=N)
    ens.load_state_dict({k: torch.from_numpy(v) for k, v in ce["params"].items()})
    ens = ens.to(DEV)
    P = dict(head.named_parameters())
    t = {k: torch.from_numpy(c[k]).to(DEV) for k in ("x", "x_next", "noise_pi", "noise_next", "a_replay", "rewards", "dones")}
    log_ent = torch.tensor([ce["log_ent_coef"]], dtype=torch.float32, device=DEV)
    gamma, sigma, clip = c["gamma"], 0.2, 0.5          # SB3's target_policy_noise and target_noise_clip

    def zero(h):
        for q in h.parameters():
            q.grad = None

    def td3_critic():
        zero(head)
        target_q = head.td_target(t["x_next"], t["rewards"], t["dones"], gamma, noise=t["noise_next"], target_policy_noise=sigma, target_noise_clip=clip)
        loss = head.critic_loss(t["x"], t["a_replay"], target_q)
        loss.backward()
        return loss

    def eager_critic():
        zero(head)
        with torch.no_grad():
            mu, _, _ = T3C.actor_forward(P, "actor_target", t["x_next"])
            an = (mu + (sigma * t["noise_next"]).clamp(-clip, clip)).clamp(-1, 1)          # SB3's TD3.train
            qn, _ = EC.critic_forward(P, "critic_target", t["x_next"], an, N)
            target_q = t["rewards"] + (1 - t["dones"]) * gamma * qn.min(dim=0)[0]
        q, _ = EC.critic_forward(P, "critic", t["x"], t["a_replay"], N)
        loss = sum(F.mse_loss(qc, target_q) for qc in q)
        loss.backward()
        return loss

    def ens_critic():
        zero(ens)
        target_q = ens.td_target(t["x_next"], t["rewards"], t["dones"], gamma, log_ent_coef=log_ent, noise=t["noise_next"])
        loss = ens.critic_loss(t["x"], t["a_replay"], target_q)
        loss.backward()
        return loss

    def td3_actor():
        zero(head)
        loss = head.actor_loss(t["x"])
        loss.backward()
        return loss

    def eager_actor():
        zero(head)
        mu, _, _ = T3C.actor_forward(P, "actor", t["x"])
        xa = torch.cat([t["x"], mu], dim=1)          # SB3's q1_forward: the first critic alone
        h = xa
        for l in range(len(ARCH[2])):
            h = torch.relu(F.linear(h, P[f"critic.qf0.{2 * l}.weight"], P[f"critic.qf0.{2 * l}.bias"]))
        loss = -F.linear(h, P[f"critic.qf0.{2 * len(ARCH[2])}.weight"], P[f"critic.qf0.{2 * len(ARCH[2])}.bias"]).mean()
        loss.backward()
        return loss

    def ens_actor():
        zero(ens)
        loss, _ = ens.actor_loss(t["x"], log_ent_coef=log_ent, noise=t["noise_pi"], q_reduce="min")
        loss.backward()
        return loss
    out = {"arch": {"features": ARCH[0], "pi": list(ARCH[1]), "qf": list(ARCH[2]), "actions": ARCH[3]}, "critics": N, "B": B,
           "target_policy_noise": sigma, "target_noise_clip": clip}
    for what, fns in (("critic_update", {"td3": td3_critic, "eager": eager_critic, "ens2": ens_critic}),
                      ("actor_update", {"td3": td3_actor, "eager": eager_actor, "ens2": ens_actor})):
        res, last = alternate(fns, a.iters, a.warmup, a.rounds)
        for name, fn in fns.items():
            res[name].update(counted(fn))
            res[name]["result_sum"] = float(last[name].detach().float().sum())
        res["td3"]["entry_points"] = entry_points(fns["td3"])
        res["td3_over_eager_call"] = round(res["td3"]["call_us"] / res["eager"]["call_us"], 3)
        res["td3_over_ens2_call"] = round(res["td3"]["call_us"] / res["ens2"]["call_us"], 3)
        out[what] = res
    print(json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=500, help="calls per timed window of (a); (b) takes ten times as many")
    ap.add_argument("--rounds", type=int, default=5, help="alternating windows per path")
    ap.add_argument("--warmup", type=int, default=30)
    ap.add_argument("--critics", type=int, default=None, help="measure the critic ensemble with this many critics (1 to 10) instead of (a) and (b)")
    ap.add_argument("--subset", type=int, default=2, help="with --critics: critics in the target's minimum (N = 2: both)")
    ap.add_argument("--q-reduce", choices=("min", "mean"), default="mean", help="with --critics: the actor loss's reduction over the critics")
    ap.add_argument("--droq", action="store_true", help="measure a critic update of the DroQ critics (N = 2, p = 0.01) against eager torch and the N = 10 ensemble")
    ap.add_argument("--tqc", action="store_true", help="measure a critic update of the TQC head (n_quantiles 25, 2 dropped per net; --critics N, default 2) against eager torch and the N = 2 ensemble")
    ap.add_argument("--td3", action="store_true", help="measure a critic update and an actor update of the TD3 head (N = 2) against eager torch and the N = 2 ensemble")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("sac_head_bench: no GPU")
    if a.droq:
        return droq(a)
    if a.tqc:
        return tqc(a)
    if a.td3:
        return td3(a)
    if a.critics is not None:
        return ensemble(a)
    out = {"arch": {"features": ARCH[0], "pi": list(ARCH[1]), "qf": list(ARCH[2]), "actions": ARCH[3]}}

    # (a) one gradient step
    c = SC.make_inputs(ARCH, 256, False, True, seed=9)
    head = m3l_amd.SACHead(ARCH[0], ARCH[3], net_arch=dict(pi=list(ARCH[1]), qf=list(ARCH[2])))
    head.load_state_dict({k: torch.from_numpy(v) for k, v in c["params"].items()})
    head = head.to(DEV)
    P = dict(head.named_parameters())
    t = {k: torch.from_numpy(c[k]).to(DEV) for k in ("x", "x_next", "noise_pi", "noise_next", "a_replay", "rewards", "dones")}
    x = t["x"].clone().requires_grad_(True)
    log_ent = torch.tensor([c["log_ent_coef"]], dtype=torch.float32, device=DEV, requires_grad=True)
    critic_params = [p for n, p in P.items() if n.startswith("critic.")]
    target_params = [p for n, p in P.items() if n.startswith("critic_target.")]
    gamma, tau, te = c["gamma"], c["tau"], c["target_entropy"]

    def zero():
        x.grad = log_ent.grad = None
        for p in head.parameters():
            p.grad = None

    def hip(read):
        zero()
        params = head.params()
        a_pi, logp = SH.action_log_prob(params, x, t["noise_pi"])
        ent_loss, ent = SH.ent_coef_loss(log_ent, logp, te)
        ent_loss.backward()
        target_q = SH.td_target(params, t["x_next"], t["rewards"], t["dones"], gamma, log_ent_coef=log_ent, noise=t["noise_next"])
        critic_loss = SH.critic_loss_from(SH.q_values(params, x, t["a_replay"]), target_q)
        critic_loss.backward()
        actor_loss = SH.actor_loss_from(logp, SH.q_values(params, x, a_pi, param_grads=False), log_ent_coef=log_ent)
        actor_loss.backward()
        head.polyak_update(tau)
        if read:
            torch.stack([ent_loss.detach(), ent, critic_loss.detach(), actor_loss.detach()]).cpu()
        return actor_loss, critic_loss

    def eager(read):
        zero()
        o = SC.actor_forward(P, x, t["noise_pi"])                                               # :303
        a_pi, log_prob = o["actions"], o["log_prob"].reshape(-1, 1)
        ent_coef = torch.exp(log_ent.detach())                                                  # :311
        ent_loss = -(log_ent * (log_prob + te).detach()).mean()                                 # :312
        if read:
            ent_loss.item(), ent_coef.item()                                                    # :313, :317
        ent_loss.backward()
        with torch.no_grad():                                                                   # :326-335
            n = SC.actor_forward(P, t["x_next"], t["noise_next"])
            qn, _ = SC.critic_forward(P, "critic_target", t["x_next"], n["actions"])
            nq = torch.min(qn.t(), dim=1, keepdim=True)[0] - ent_coef * n["log_prob"].reshape(-1, 1)
            target_q = t["rewards"].reshape(-1, 1) + (1 - t["dones"].reshape(-1, 1)) * gamma * nq
        q, _ = SC.critic_forward(P, "critic", x, t["a_replay"])                                 # :339
        critic_loss = 0.5 * sum(F.mse_loss(qc.reshape(-1, 1), target_q) for qc in q)            # :342
        if read:
            critic_loss.item()                                                                  # :344
        critic_loss.backward()
        for p in critic_params:                                                                 # :347 of the next step
            p.grad = None
        qp, _ = SC.critic_forward(P, "critic", x, a_pi)                                         # :354
        actor_loss = (ent_coef * log_prob - torch.min(qp.t(), dim=1, keepdim=True)[0]).mean()   # :356
        if read:
            actor_loss.item()                                                                   # :357
        actor_loss.backward()
        with torch.no_grad():                                                                   # :366, SB3's polyak_update
            for p, tp in zip(critic_params, target_params):
                tp.mul_(1 - tau)
                torch.add(tp, p, alpha=tau, out=tp)
        return actor_loss, critic_loss
    fns = {"hip": lambda: hip(False), "eager": lambda: eager(False), "hip_values_read": lambda: hip(True), "eager_values_read": lambda: eager(True)}
    res, last = alternate(fns, a.iters, a.warmup, a.rounds)
    for name, fn in fns.items():
        res[name].update(counted(fn))
        res[name]["actor_loss"], res[name]["critic_loss"] = float(last[name][0].detach()), float(last[name][1].detach())
    res["hip"]["entry_points"] = entry_points(fns["hip"])
    res["hip_over_eager_call"] = round(res["hip"]["call_us"] / res["eager"]["call_us"], 3)
    res["hip_over_eager_call_values_read"] = round(res["hip_values_read"]["call_us"] / res["eager_values_read"]["call_us"], 3)
    out["gradient_step_B256"] = res

    # (b) one environment step
    xb = torch.randn(8, ARCH[0], generator=torch.Generator().manual_seed(3)).to(DEV)
    noise = torch.randn(8, ARCH[3], generator=torch.Generator().manual_seed(4)).to(DEV)

    def hip_act():
        return head(xb, noise=noise)

    def eager_act():
        with torch.no_grad():          # SB3's Actor.forward: the action alone, no log-probability
            h = xb
            for l in range(len(ARCH[1])):
                h = torch.relu(F.linear(h, P[f"actor.latent_pi.{2 * l}.weight"], P[f"actor.latent_pi.{2 * l}.bias"]))
            mu = F.linear(h, P["actor.mu.weight"], P["actor.mu.bias"])
            s = torch.clamp(F.linear(h, P["actor.log_std.weight"], P["actor.log_std.bias"]), SC.LOG_STD_MIN, SC.LOG_STD_MAX)
            return torch.tanh(mu + s.exp() * noise)
    fns = {"hip": hip_act, "eager": eager_act}
    res, last = alternate(fns, 10 * a.iters, a.warmup, a.rounds)
    for name, fn in fns.items():
        res[name].update(counted(fn))
        res[name]["actions_sum"] = float(last[name].sum())
    res["hip"]["entry_points"] = entry_points(hip_act)
    res["hip_over_eager_call"] = round(res["hip"]["call_us"] / res["eager"]["call_us"], 3)
    out["actor_no_grad_B8"] = res
    print(json.dumps(out))


if __name__ == "__main__":
    main()
