"""CPU checks of the TD3 head's restatement (tests/td3_cases.py), of its inputs' conditions, and of everything in m3l_amd/td3.py that needs no
device: the names, `TD3Params.from_policy`, and every refusal that comes before a launch."""
import math
import os
import types

import numpy as np
import pytest
import torch
from torch import nn

import m3l_amd
import sac_ens_cases as EC
import td3_cases as TC
from m3l_amd import _lib as L
from m3l_amd import td3 as T3

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_the_package_exports_the_head_and_the_library_its_entries():
    assert m3l_amd.TD3Head is T3.TD3Head and m3l_amd.TD3Params is T3.TD3Params and "TD3Head" in m3l_amd.__all__ and "TD3Params" in m3l_amd.__all__
    hdr = open(os.path.join(ROOT, "include", "m3l_amd.h")).read()
    assert "TD3 head (ABI 422)" in hdr
    lib = L.lib()
    assert lib.m3l_version() >= 422
    for fn in ("m3l_td3_ws_bytes", "m3l_td3_actor_fwd", "m3l_td3_actor_bwd", "m3l_td3_td_target", "m3l_td3_critic_loss_fwd", "m3l_td3_actor_loss_fwd"):
        assert fn in L.EXPORTS and fn + "(" in hdr and hasattr(lib, fn)


@pytest.mark.parametrize("name", list(TC.CASES))
def test_input_conditions(name):
    """What the float32 / float64 comparisons rest on: the margins on every gate, tie and clamp edge, and entries on both sides of each clamp in
    every noise tensor and mode; the actor and its target differ; everything is float32."""
    c = TC.case(name)
    cond = TC.check(c)
    print(f"[{name}] gate {cond['gate']:.2e} tie {cond['tie']:.2e} clamp {cond['clamp']:.2e}")
    assert cond["gate"] >= TC.GATE_MARGIN and cond["tie"] >= TC.TIE_MARGIN and cond["clamp"] >= TC.CLAMP_MARGIN
    assert set(cond["sides"]) == {(ev, m) for ev in TC.EVALS for m in TC.NOISY}
    for (ev, m), s in cond["sides"].items():
        assert s["outer_out"] >= 1, (ev, m)
        if m == "clip":
            assert s["inner_out"] >= 1 and s["inner_in"] >= 1, (ev, m)
    assert all(v.dtype == np.float32 for v in c["params"].values()) and list(c["params"]) == TC.param_names(c["arch"], c["n_critics"])
    assert all(not np.array_equal(c["params"][k], c["params"][k.replace("actor.", "actor_target.", 1)]) for k in TC.actor_names(c["arch"]))
    ref = TC.reference(name)
    for m in TC.MODES:
        for ev in TC.EVALS:
            assert np.abs(ref["a"][m][ev]).max() <= 1.0
    assert np.array_equal(ref["a"]["det"]["pi"], ref["mu"]["pi"])


def _loop_actor(P, prefix, x):
    """mu of one row, Linear by Linear, unit by unit."""
    h, l = [float(v) for v in x], 0
    while True:
        W, b = np.asarray(P[f"{prefix}.mu.{2 * l}.weight"], dtype=np.float64), np.asarray(P[f"{prefix}.mu.{2 * l}.bias"], dtype=np.float64)
        z = [sum(W[j, k] * h[k] for k in range(len(h))) + b[j] for j in range(W.shape[0])]
        if f"{prefix}.mu.{2 * l + 2}.weight" not in P:
            return [math.tanh(v) for v in z]
        h, l = [max(v, 0.0) for v in z], l + 1


def _loop_critic(P, prefix, i, xa):
    h, l = list(xa), 0
    while True:
        W, b = np.asarray(P[f"{prefix}.qf{i}.{2 * l}.weight"], dtype=np.float64), np.asarray(P[f"{prefix}.qf{i}.{2 * l}.bias"], dtype=np.float64)
        z = [sum(W[j, k] * h[k] for k in range(len(h))) + b[j] for j in range(W.shape[0])]
        if f"{prefix}.qf{i}.{2 * l + 2}.weight" not in P:
            return z[0]
        h, l = [max(v, 0.0) for v in z], l + 1


def _loop_smooth(a, n, sigma, clip):
    e = sigma * n
    if clip is not None:
        e = min(max(e, -clip), clip)
    return min(max(a + e, -1.0), 1.0)


@pytest.mark.parametrize("name", ["a64_n3_b3", "nohid_n10_b3", "f16a7_n10_b1", "mixed_n3_b33"])
def test_the_restatement_against_a_loop_written_version(name):
    """Row by row, critic by critic, in Python floats: the actions, the target (both actors, every mode, per-row discounts), the critic loss
    with its coefficients and td errors, the three actor losses."""
    c, ref = TC.case(name), TC.reference(name)
    P, N, B = c["params"], c["n_critics"], c["x"].shape[0]
    w, disc = c["weights"].astype(np.float64), c["discounts"].astype(np.float64)
    for mode, (sigma, clip) in TC.MODES.items():
        acts = {}
        for ev, (prefix, xk, nk) in TC.EVALS.items():
            acts[ev] = [[_loop_smooth(a, float(n), sigma, clip) for a, n in zip(_loop_actor(P, prefix, c[xk][r]), c[nk][r])] for r in range(B)]
            assert np.allclose(acts[ev], ref["a"][mode][ev], rtol=0, atol=1e-12)
        for online in (False, True):
            ev = "next_online" if online else "next"
            tq = []
            for r in range(B):
                xa = [float(v) for v in c["x_next"][r]] + acts[ev][r]
                m = min(_loop_critic(P, "critic_target", i, xa) for i in range(N))
                tq.append(float(c["rewards"][r]) + (1.0 - float(c["dones"][r])) * disc[r] * m)
            assert np.allclose(tq, TC.target_ref(c, ref, mode, c["discounts"], online), rtol=1e-12, atol=1e-12)
        q = [[_loop_critic(P, "critic", i, [float(v) for v in c["x"][r]] + acts["pi"][r]) for r in range(B)] for i in range(N)]
        for reduce, red in (("first", lambda col: col[0]), ("min", min), ("mean", lambda col: sum(col) / N)):
            loss = -sum(red([q[i][r] for i in range(N)]) for r in range(B)) / B
            assert np.allclose(loss, TC.actor_loss_ref(c, reduce, mode)["loss"], rtol=1e-12, atol=1e-12)
    t = TC.target_ref(c, ref, "clip", c["gamma"])
    qr = [[_loop_critic(P, "critic", i, [float(v) for v in c["x"][r]] + [float(v) for v in c["a_replay"][r]]) for r in range(B)] for i in range(N)]
    for weights in (None, c["weights"]):
        got = TC.critic_loss_ref(c, t, weights)
        wr = np.ones(B) if weights is None else w
        assert np.allclose(sum(sum(wr[r] * (qr[i][r] - t[r]) ** 2 for r in range(B)) / B for i in range(N)), got["loss"], rtol=1e-12)
        assert np.allclose([[2.0 * wr[r] * (qr[i][r] - t[r]) / B for r in range(B)] for i in range(N)], got["coef"], rtol=1e-10, atol=1e-14)
        assert np.allclose([sum(abs(qr[i][r] - t[r]) for i in range(N)) / N for r in range(B)], got["td_abs"], rtol=1e-12)
        twice = EC.critic_loss_ref(dict(c, params={k: v for k, v in c["params"].items() if not k.startswith("actor")}), t, weights)
        assert np.allclose(got["loss"], 2.0 * twice["loss"], rtol=1e-14) and all(np.allclose(got["grad"][k], 2.0 * g, rtol=1e-12, atol=1e-300) for k, g in twice["grad"].items())


def _tiny():
    """F = 2, A = 1, an actor and one critic without hidden layers, two rows: everything below is worked out by hand."""
    f32 = lambda *v: np.asarray(v, dtype=np.float32)      # noqa: E731
    P = {"actor.mu.0.weight": f32([0.5, -1.0]), "actor.mu.0.bias": f32(0.25), "actor_target.mu.0.weight": f32([1.0, 0.5]), "actor_target.mu.0.bias": f32(-0.5),
         "critic.qf0.0.weight": f32([1.0, 2.0, -3.0]), "critic.qf0.0.bias": f32(0.5), "critic_target.qf0.0.weight": f32([0.5, -1.0, 2.0]),
         "critic_target.qf0.0.bias": f32(1.0)}
    return dict(params=P, arch=(2, (), (), 1), n_critics=1, x=f32([1.0, 0.5], [-2.0, 1.0]), x_next=f32([0.5, 1.0], [2.0, 2.0]), noise_pi=f32([0.25], [-4.0]),
                noise_next=f32([2.0], [0.5]), noise_next_online=f32([0.0], [0.0]), a_replay=f32([0.5], [-0.5]), rewards=f32(1.0, -1.0), dones=f32(0.0, 1.0),
                weights=f32(1.0, 1.0), discounts=f32(0.5, 0.5), gamma=0.5, tau=0.25)


def test_a_two_row_example_worked_out_by_hand():
    c = _tiny()
    ref = TC.forward_ref(c)
    sigma, clip = TC.MODES["clip"]          # 0.6, 0.5
    # the actor at x: pre = 0.5 x0 - x1 + 0.25 -> 0.25 and -1.75
    mu = [math.tanh(0.25), math.tanh(-1.75)]
    assert np.allclose(ref["mu"]["pi"].ravel(), mu, atol=1e-15)
    # row 0: 0.6 * 0.25 = 0.15 inside the clip; row 1: 0.6 * -4 = -2.4 -> -0.5, and tanh(-1.75) - 0.5 < -1 -> -1
    a = [mu[0] + 0.15, -1.0]
    assert mu[1] - 0.5 < -1.0 and np.allclose(ref["a"]["clip"]["pi"].ravel(), a, atol=1e-15)
    assert np.allclose(ref["a"]["noclip"]["pi"].ravel(), [mu[0] + 0.15, -1.0], atol=1e-15)
    # the target actor at x': pre = x0 + 0.5 x1 - 0.5 -> 0.5 and 2.5; noise 0.6 * 2 = 1.2 -> 0.5, and 0.6 * 0.5 = 0.3: tanh(2.5) + 0.3 > 1 -> 1
    an = [math.tanh(0.5) + 0.5, 1.0]
    assert math.tanh(0.5) + 0.5 < 1.0 < math.tanh(2.5) + 0.3 and np.allclose(ref["a"]["clip"]["next"].ravel(), an, atol=1e-15)
    # the target critic: q = 0.5 x0 - x1 + 2 a + 1;  target = r + (1 - done) 0.5 q: row 1 is done
    qn = [0.25 - 1.0 + 2.0 * an[0] + 1.0, 1.0 - 2.0 + 2.0 + 1.0]
    tq = [1.0 + 0.5 * qn[0], -1.0]
    assert np.allclose(TC.target_ref(c, ref, "clip", 0.5), tq, atol=1e-15) and TC.target_ref(c, ref, "clip", 0.5)[1] == -1.0
    # the critic at (x, a_replay): q = x0 + 2 x1 - 3 a + 0.5 -> 1 and 2;  loss = mean (q - t)^2 (one critic), coef = 2 (q - t) / 2
    qr = [1.0 + 1.0 - 1.5 + 0.5, -2.0 + 2.0 + 1.5 + 0.5]
    cl = TC.critic_loss_ref(c, np.asarray(tq))
    assert np.allclose(cl["loss"], ((qr[0] - tq[0]) ** 2 + (qr[1] - tq[1]) ** 2) / 2, atol=1e-14)
    assert np.allclose(cl["coef"], [[qr[0] - tq[0], qr[1] - tq[1]]], atol=1e-14) and np.allclose(cl["td_abs"], [abs(qr[0] - tq[0]), abs(qr[1] - tq[1])])
    assert np.allclose(cl["grad"]["critic.qf0.0.bias"], (qr[0] - tq[0]) + (qr[1] - tq[1]), atol=1e-14)
    # the actor loss on the clipped noisy actions: -mean q(x, a), dq / da = -3; both clamps pass the gradient: d pre = (3 / 2) (1 - mu^2) on BOTH
    # rows, though row 1's action sits on the edge
    al = TC.actor_loss_ref(c, "min", "clip")
    q = [1.0 + 1.0 - 3.0 * a[0] + 0.5, -2.0 + 2.0 - 3.0 * a[1] + 0.5]
    dpre = [1.5 * (1.0 - mu[0] ** 2), 1.5 * (1.0 - mu[1] ** 2)]
    assert np.allclose(al["loss"], -(q[0] + q[1]) / 2, atol=1e-14) and np.allclose(al["grad"]["actor.mu.0.bias"], dpre[0] + dpre[1], atol=1e-14)
    assert np.allclose(al["grad"]["actor.mu.0.weight"], [dpre[0] * 1.0 + dpre[1] * -2.0, dpre[0] * 0.5 + dpre[1] * 1.0], atol=1e-14)
    assert np.allclose(al["grad"]["x"], [[dpre[0] * 0.5, dpre[0] * -1.0], [dpre[1] * 0.5, dpre[1] * -1.0]], atol=1e-14)
    assert np.allclose(TC.actions_ref(c, "clip", np.ones((2, 1)))["grad"]["actor.mu.0.bias"], (dpre[0] + dpre[1]) / 1.5, atol=1e-14)
    # Polyak, tau = 0.25, on both target nets
    pk = TC.polyak_ref(c)
    assert np.allclose(pk["actor_target.mu.0.bias"], 0.75 * -0.5 + 0.25 * 0.25) and np.allclose(pk["critic_target.qf0.0.weight"], [0.625, -0.25, 0.75])
    assert set(pk) == {k for k in c["params"] if "_target." in k}


def test_the_step_is_its_parts_in_order():
    c = TC.case(TC.ANCHOR)
    s, ref = TC.step_ref(c), TC.reference(TC.ANCHOR)
    t = TC.target_ref(c, ref, "clip", c["gamma"])
    assert np.array_equal(s["target_q"], t) and s["critic_loss"] == TC.critic_loss_ref(c, t)["loss"] and s["actor_loss"] == TC.actor_loss_ref(c, "first")["loss"]
    assert set(s["grad"]) == set(TC.actor_names(c["arch"]) + EC.critic_names(c["arch"], 2) + ["x"]) and set(s["target"]) == {k for k in c["params"] if "_target." in k}
    # in det mode the actions' gradient is the true derivative: a directional finite difference agrees
    g = TC.actions_ref(c, "det", np.ones_like(c["noise_pi"], dtype=np.float64))["grad"]
    rng = np.random.default_rng(0)
    d = rng.standard_normal(c["x"].shape)
    f = lambda eps: TC.actor_forward(TC.as_torch(c["params"]), "actor", torch.from_numpy(c["x"].astype(np.float64) + eps * d))[0].sum().item()      # noqa: E731
    assert abs((f(1e-6) - f(-1e-6)) / 2e-6 - float((g["x"] * d).sum())) <= 1e-6 * max(1.0, abs(float((g["x"] * d).sum())))


@pytest.mark.parametrize("arch,N", [("a64", 2), ("nohid", 10), ("amax", 1), ("mixed", 3)])
def test_state_dict_names_in_creation_order(arch, N):
    Fd, pi, qf, A = TC.ARCHS[arch]
    head = m3l_amd.TD3Head(Fd, A, net_arch=dict(pi=list(pi), qf=list(qf)), n_critics=N)
    assert list(head.state_dict()) == TC.param_names(TC.ARCHS[arch], N)
    assert isinstance(head.actor.mu[-1], nn.Tanh) and isinstance(head.actor.mu[-2], nn.Linear) and head.actor.mu[-2].out_features == A
    for part in ("actor", "critic"):
        live, target = getattr(head, part), getattr(head, part + "_target")
        assert all(torch.equal(a, b) and a.requires_grad and not b.requires_grad for a, b in zip(live.parameters(), target.parameters()))
    sd = {k: torch.randn_like(v) for k, v in head.state_dict().items()}
    head.load_state_dict(sd, strict=True)
    p = head.params()
    assert p.n_critics == N and len(p.actor_flat()) == len(p.actor_flat(True)) == 2 * (len(pi) + 1) and len(p.critic_flat()) == 2 * N * (len(qf) + 1)
    assert p.mu[0] is head.actor.mu[-2].weight and p.mu_target[1] is head.actor_target.mu[-2].bias and p.qf_target[N - 1][-1][0] is getattr(head.critic_target, f"qf{N - 1}")[-1].weight
    assert T3._arch(Fd, p) == (Fd, A, tuple(pi), tuple(qf))
    default = m3l_amd.TD3Head(32, 2)
    assert T3._arch(32, default.params()) == (32, 2, (256, 256), (256, 256)) and default.n_critics == 2


class _StandIn:
    """What `from_policy` reads of SB3's TD3Policy: the attribute names, nothing else of SB3."""

    def __init__(self, n=2, F=16, A=3, w=32):
        net = lambda: types.SimpleNamespace(mu=nn.Sequential(nn.Linear(F, w), nn.ReLU(), nn.Linear(w, A), nn.Tanh()))      # noqa: E731
        crit = lambda: types.SimpleNamespace(n_critics=n, share_features_extractor=True,      # noqa: E731
                                             **{f"qf{i}": nn.Sequential(nn.Linear(F + A, w), nn.ReLU(), nn.Linear(w, 1)) for i in range(n)})
        self.actor, self.actor_target, self.critic, self.critic_target = net(), net(), crit(), crit()
        self.share_features_extractor = True


def test_from_policy_reads_a_stand_in_with_sb3s_names():
    pol = _StandIn(n=3)
    p = m3l_amd.TD3Params.from_policy(pol)
    assert p.n_critics == 3 and p.pi[0][0] is pol.actor.mu[0].weight and p.mu[0] is pol.actor.mu[2].weight and p.mu_target[0] is pol.actor_target.mu[2].weight
    assert p.qf[2][1][1] is pol.critic.qf2[2].bias and p.qf_target[0][0][0] is pol.critic_target.qf0[0].weight
    assert T3._arch(16, p) == (16, 3, (32,), (32,))

    def broken(change):
        q = _StandIn(n=2)
        change(q)
        return q
    for change in (lambda q: setattr(q, "share_features_extractor", False), lambda q: setattr(q.critic, "share_features_extractor", False),
                   lambda q: setattr(q.critic, "n_critics", 3), lambda q: delattr(q.critic_target, "qf1"),
                   lambda q: setattr(q.actor, "mu", nn.Sequential(nn.Linear(16, 3))), lambda q: setattr(q.actor, "mu", nn.Sequential(nn.Linear(16, 3), nn.ReLU())),
                   lambda q: setattr(q.actor_target, "mu", nn.Sequential(nn.Linear(16, 32), nn.Tanh(), nn.Linear(32, 3), nn.Tanh())),
                   lambda q: setattr(q.actor, "mu", nn.Sequential(nn.Linear(16, 3, bias=False), nn.Tanh())),
                   lambda q: setattr(q.critic, "qf0", nn.Sequential(nn.Linear(19, 32), nn.Tanh(), nn.Linear(32, 1))),
                   lambda q: setattr(q.critic, "qf1", nn.Sequential(nn.Linear(19, 2)))):
        with pytest.raises(ValueError):
            m3l_amd.TD3Params.from_policy(broken(change))
    for change in (lambda q: setattr(q.critic, "qf1", nn.Sequential(nn.Linear(19, 48), nn.ReLU(), nn.Linear(48, 1))),      # critics that differ
                   lambda q: setattr(q.critic_target, "qf0", nn.Sequential(nn.Linear(19, 1))),                              # a target unlike its critic
                   lambda q: setattr(q.actor_target, "mu", nn.Sequential(nn.Linear(16, 3), nn.Tanh())),                      # a target actor unlike the actor
                   lambda q: q.critic.qf0.double(), lambda q: q.actor.mu.half(),
                   lambda q: setattr(q.actor, "mu", nn.Sequential(nn.Linear(16, 24), nn.ReLU(), nn.Linear(24, 3), nn.Tanh()))):      # a width off the rule
        with pytest.raises(ValueError):
            T3._arch(16, m3l_amd.TD3Params.from_policy(broken(change)))


def test_refusals_that_need_no_device():
    ok = dict(features_dim=64, action_dim=3)
    for kw in (dict(net_arch=[400, 300]), dict(net_arch=[24]), dict(net_arch=[528]), dict(features_dim=40), dict(net_arch=[64] * 4),
               dict(net_arch=dict(pi=[64], qf=[64] * 4)), dict(action_dim=0), dict(action_dim=65), dict(action_dim=2.5), dict(n_critics=0), dict(n_critics=11),
               dict(n_critics=True), dict(n_critics=2.0), dict(activation_fn=nn.Tanh), dict(share_features_extractor=False)):
        with pytest.raises(ValueError):
            m3l_amd.TD3Head(**{**ok, **kw})
    with pytest.raises(ValueError, match=r"\[400, 300\].*\[256, 256\]"):
        m3l_amd.TD3Head(64, 3, net_arch=[400, 300])
    head = m3l_amd.TD3Head(64, 3, net_arch=[64])
    x, v, a, n = torch.zeros(5, 64), torch.zeros(5), torch.zeros(5, 3), torch.zeros(5, 3)
    for call in (lambda: head.actions(x, noise=n, noise_std=-0.1), lambda: head.actions(x, noise=n, noise_std=float("inf")), lambda: head.actions(x, noise=n, noise_std=None),
                 lambda: head.actions(x, noise=n, noise_std=0.1, noise_clip=0.0), lambda: head.actions(x, noise=n, noise_std=0.1, noise_clip=-0.5),
                 lambda: head.actions(x, noise=n, noise_std=0.1, noise_clip=float("nan")), lambda: head(x, noise=n, noise_std=-1.0),
                 lambda: head.td_target(x, v, v, 0.99, target_policy_noise=-0.2), lambda: head.td_target(x, v, v, 0.99, target_policy_noise=float("nan")),
                 lambda: head.td_target(x, v, v, 0.99, target_noise_clip=0.0), lambda: head.td_target(x, v, v, 0.99, target_noise_clip=-1.0),
                 lambda: head.actor_loss(x, q_reduce="max"), lambda: head.actor_loss(x, q_reduce=None), lambda: head.actor_loss(x, noise_std=-1.0)):
        with pytest.raises(ValueError):
            call()
    # past the argument checks a CPU tensor is an error of its own: there is no eager fallback
    for call in (lambda: head(x), lambda: head.actions(x), lambda: head.q_values(x, a), lambda: head.td_target(x, v, v, 0.99), lambda: head.critic_loss(x, a, v),
                 lambda: head.actor_loss(x), lambda: head.polyak_update(0.005)):
        with pytest.raises(m3l_amd.M3LError):
            call()
