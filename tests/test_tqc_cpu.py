"""CPU-only checks of the TQC head: the C ABI declarations and descriptor packing, the public surface (TQCHead: sb3-contrib's names, every
refusal that needs no device), and the float64 restatement of tests/tqc_cases.py against a second, loop-written version of the sort / keep rule
and of the quantile-Huber loss, its gradient against the header's closed form, and one example computed by hand.  No kernel is launched here."""
import ctypes as C
import os

import numpy as np
import pytest
import torch
from torch import nn

import m3l_amd
import tqc_cases as TC
from m3l_amd import TQCHead
from m3l_amd import _lib as L
from m3l_amd import tqc as TQ

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ["m3l_tqc_ws_bytes", "m3l_tqc_critic_fwd", "m3l_tqc_critic_bwd", "m3l_tqc_td_target", "m3l_tqc_loss_ws_bytes", "m3l_tqc_critic_loss_fwd",
           "m3l_tqc_actor_loss_fwd"]


def _head(name):
    Fd, qf, A, N, nq, d, _ = TC.CASES[name]
    return TQCHead(Fd, A, net_arch=dict(pi=list(TC.PI), qf=list(qf)), n_critics=N, n_quantiles=nq, top_quantiles_to_drop_per_net=d)


def test_symbols_are_declared_bound_and_versioned():
    hdr = open(os.path.join(ROOT, "include", "m3l_amd.h")).read()
    for s in SYMBOLS:
        assert s + "(" in hdr and s in L.EXPORTS and hasattr(L.lib(), s), s
    assert "typedef struct m3l_tqc_desc" in hdr and "SAC TQC critics (ABI 421)" in hdr and "M3L_TQC_MAX_POOL 512" in hdr
    section = hdr.split("(ABI 421)")[1].split("typedef struct")[0]
    for word in ("parity unpinned", "sum_over_quantiles", "rank", "NaN", "7 launches", "M3L_TQC_MAX_POOL", "115 328"):
        assert word in section, word
    lib = L.lib()
    assert lib.m3l_version() >= 421 and L.TQC_MAX_POOL == TQ.MAX_POOL == 512 and L.TQC_MAX_QUANTILES == TQ.MAX_QUANTILES == 64
    assert [n for n, _ in L.TqcDesc._fields_] == ["ens", "n_quantiles", "top_quantiles_to_drop"]
    assert L.TqcDesc.n_quantiles.offset == C.sizeof(L.SacEnsDesc) == 768 and L.TqcDesc.top_quantiles_to_drop.offset == 772 and C.sizeof(L.TqcDesc) == 776
    d = L.TqcDesc()
    d.ens.features, d.ens.actions, d.ens.n_pi, d.ens.n_qf, d.ens.n_critics, d.n_quantiles, d.top_quantiles_to_drop = 256, 7, 2, 2, 2, 25, 2
    for l in range(2):
        d.ens.pi_width[l] = d.ens.qf_width[l] = 256
    ens = lib.m3l_sac_ens_ws_bytes(C.byref(d.ens), 256)
    # the ensemble's workspace with d z [N, B, nq] where it keeps d q [N, B]
    assert lib.m3l_tqc_ws_bytes(C.byref(d), 256) == ens + 4 * 2 * 256 * 24
    assert lib.m3l_tqc_loss_ws_bytes(2, 37) == 4 * (2 * 3 + 2 * 37) and lib.m3l_tqc_loss_ws_bytes(0, 37) == 256 == lib.m3l_tqc_loss_ws_bytes(11, 37)
    for field, bad, why in (("n_quantiles", 0, "n_quantiles"), ("n_quantiles", 65, "n_quantiles"), ("top_quantiles_to_drop", 25, "top_quantiles_to_drop"),
                            ("top_quantiles_to_drop", -1, "top_quantiles_to_drop")):
        keep = getattr(d, field)
        setattr(d, field, bad)
        assert lib.m3l_tqc_ws_bytes(C.byref(d), 256) == 256, (field, bad)          # an unsupported shape sizes nothing
        assert lib.m3l_tqc_critic_fwd(C.byref(d), 256, None, None, None, None, None) != 0 and why in L.last_error(), L.last_error()
        setattr(d, field, keep)
    d.ens.n_critics, d.n_quantiles = 9, 64          # a pool beyond the limit: both numbers are named
    assert lib.m3l_tqc_td_target(C.byref(d), 256, None, None, None, None, None, 0.99, 0.1, None, None, None) != 0
    assert "576" in L.last_error() and "512" in L.last_error(), L.last_error()
    d.ens.n_critics = 8
    assert lib.m3l_tqc_ws_bytes(C.byref(d), 256) > 256


def test_descriptor_packing():
    name = "f16_a7_q48x32_n3q5d4_b37"
    head = _head(name)
    p = head.params()
    named = dict(head.named_parameters())
    arch = TC.arch_of(name)
    assert (p.n_critics, p.n_quantiles, p.top_quantiles_to_drop_per_net, p.n_target_quantiles, len(p)) == (3, 5, 4, 3, 5)
    assert [t.data_ptr() for t in p.critic_flat()] == [named[n].data_ptr() for n in TC.critic_names(arch, 3)]
    assert [t.data_ptr() for t in p.critic_flat(True)] == [named[n].data_ptr() for n in TC.critic_names(arch, 3, "critic_target")]
    a = TQ._arch(16, p)
    assert a == (16, 7, (32,), (48, 32))
    d = TQ._desc(a, p, actor=p.actor_flat(), critic=p.critic_flat(True))
    assert (d.ens.features, d.ens.actions, d.ens.n_qf, d.ens.n_critics, d.n_quantiles, d.top_quantiles_to_drop) == (16, 7, 2, 3, 5, 4)
    for c in range(3):
        net = getattr(head.critic_target, f"qf{c}")
        assert d.ens.q_weight[c] == net[4].weight.data_ptr() and d.ens.q_bias[c] == net[4].bias.data_ptr() and tuple(net[4].weight.shape) == (5, 32)
    assert d.ens.q_weight[3] is None and d.ens.mu_weight == head.actor.mu.weight.data_ptr()


@pytest.mark.parametrize("name", list(TC.CASES))
def test_state_dict_names_shapes_and_k(name):
    """sb3-contrib's key names in creation order, every shape, the attributes of `critic`, K, and a strict load of the case's parameters and of
    the torch.nn restatement's state dict; the target starts as a frozen copy."""
    Fd, qf, A, N, nq, d, B = TC.CASES[name]
    arch, c = TC.arch_of(name), TC.case(name)
    head = _head(name)
    sd = head.state_dict()
    assert list(sd.keys()) == TC.param_names(arch, N) == list(c["params"])
    assert [tuple(v.shape) for v in sd.values()] == [tuple(v.shape) for v in c["params"].values()]
    k = qf[-1] if qf else Fd + A
    for sub in (head.critic, head.critic_target):
        assert (sub.n_critics, sub.n_quantiles, sub.quantiles_total) == (N, nq, N * nq) and not hasattr(sub, f"qf{N}")
        assert all(tuple(getattr(sub, f"qf{i}")[2 * len(qf)].weight.shape) == (nq, k) for i in range(N))
    assert head.n_target_quantiles == head.params().n_target_quantiles == c["K"] == TC.kept(N, nq, d) == N * (nq - d)
    for key in TC.critic_names(arch, N):
        assert torch.equal(sd[key], sd["critic_target." + key[len("critic."):]])
    assert [key for key, t in head.named_parameters() if t.requires_grad] == TC.param_names(arch, N)[:len(sd) - len(TC.critic_names(arch, N))]
    head.load_state_dict({key: torch.from_numpy(np.asarray(v)) for key, v in c["params"].items()}, strict=True)
    ref = TC.as_modules(c, torch.float32)
    head.load_state_dict(ref.state_dict(), strict=True)
    p = TQ.TQCParams.from_policy(ref, top_quantiles_to_drop_per_net=d)          # an sb3-contrib-like object is read the same way
    assert (p.n_critics, p.n_quantiles, p.n_target_quantiles) == (N, nq, c["K"])
    assert "TQCHead" in m3l_amd.__all__ and "TQCParams" in m3l_amd.__all__


def test_default_architecture():
    head = TQCHead(256, 7)
    assert (head.n_critics, head.n_quantiles, head.top_quantiles_to_drop_per_net, head.n_target_quantiles) == (2, 25, 2, 46)
    assert [tuple(p.shape) for p in head.critic.qf1.parameters()] == [(256, 263), (256,), (256, 256), (256,), (25, 256), (25,)]
    assert [tuple(p.shape) for p in head.actor.parameters()] == [(256, 256), (256,), (256, 256), (256,), (7, 256), (7,), (7, 256), (7,)]


def test_every_refusal_that_needs_no_device():
    for bad in (0, 11, -1, 2.5, "3", True, None):
        with pytest.raises(ValueError, match="from 1 to 10"):
            TQCHead(64, 3, n_critics=bad)
    for bad in (0, 65, -1, 2.5, 25.0, "25", True, None):
        with pytest.raises(ValueError, match="n_quantiles"):
            TQCHead(64, 3, n_quantiles=bad)
    for nq, bad in ((25, 25), (25, -1), (25, 30), (1, 1), (25, 1.0), (25, "2"), (25, True), (25, None)):
        with pytest.raises(ValueError, match="top_quantiles_to_drop_per_net"):
            TQCHead(64, 3, n_quantiles=nq, top_quantiles_to_drop_per_net=bad)
    for n, nq in ((10, 64), (9, 57), (10, 52)):          # a pool beyond the target kernel's LDS budget: both numbers are in the message
        with pytest.raises(ValueError, match=f"{n * nq} pooled.*at most 512"):
            TQCHead(64, 3, n_critics=n, n_quantiles=nq)
    for n, nq in ((10, 25), (5, 64), (8, 64), (10, 51)):          # what the limit admits
        assert TQCHead(16, 1, net_arch=[16], n_critics=n, n_quantiles=nq).critic.quantiles_total == n * nq
    # SACEnsembleHead's refusals, by its helpers
    for kw, why in ((dict(features_dim=40), "multiples of 16"), (dict(net_arch=dict(pi=[64], qf=[1024])), "at most 512"), (dict(action_dim=65), "1 to 64"),
                    (dict(net_arch=dict(pi=[16], qf=[16] * 4)), "0 to 3 hidden layers"), (dict(activation_fn=nn.Tanh), "ReLU only"),
                    (dict(use_sde=True), "use_sde"), (dict(share_features_extractor=False), "share_features_extractor=False")):
        args = dict(features_dim=64, action_dim=3)
        args.update(kw)
        with pytest.raises(ValueError, match=why):
            TQCHead(**args)
    with pytest.raises(TypeError):          # what is out of scope has no argument
        TQCHead(64, 3, critic_layer_norm=True)
    # from_policy on modules that do not fit
    FP = TQ.TQCParams.from_policy
    mk = lambda **kw: TQCHead(64, 3, net_arch=dict(pi=[64], qf=[64]), n_critics=3, n_quantiles=5, **kw)      # noqa: E731
    m = mk()
    m.critic.qf2 = TQCHead(64, 3, net_arch=dict(pi=[64], qf=[32]), n_critics=1, n_quantiles=5).critic.qf0
    with pytest.raises(ValueError, match="must be alike"):
        TQ._arch(64, FP(m))
    m = mk()
    del m.critic_target.qf2
    with pytest.raises(ValueError, match="must agree|n_critics"):
        FP(m)
    m = mk()
    m.critic.qf1 = TQCHead(64, 3, net_arch=dict(pi=[64], qf=[64]), n_critics=1, n_quantiles=7).critic.qf0
    with pytest.raises(ValueError, match=r"nn.Linear\(., 5\)"):
        FP(m)
    m = mk()
    m.critic.qf0[1] = nn.Tanh()
    with pytest.raises(ValueError, match="ReLU only"):
        FP(m)
    m = mk()
    m.critic.qf0 = m3l_amd.SACEnsembleHead(64, 3, net_arch=dict(pi=[64], qf=[64]), n_critics=1, critic_layer_norm=True).critic.qf0
    with pytest.raises(ValueError):          # LayerNorm critics are not computed under TQC
        FP(m)
    m = mk()
    m.actor.use_sde = True
    with pytest.raises(ValueError, match="use_sde"):
        FP(m)
    bare = TC.as_modules(TC.case(TC.STEP), torch.float32)
    with pytest.raises(ValueError, match="pass it"):
        FP(bare)
    # argument forms that are refused before any tensor is looked at
    head = mk()
    x, a = torch.zeros(4, 64), torch.zeros(4, 3)
    for bad in (torch.zeros(4), torch.zeros(4, 8), torch.zeros(4, 10), torch.zeros(4, 9, 1)):
        with pytest.raises(ValueError, match=r"K = 9"):
            head.critic_loss(x, a, bad)


def test_cpu_tensors_raise_and_nothing_falls_back():
    head = TQCHead(64, 3, net_arch=dict(pi=[64], qf=[64]), n_critics=3, n_quantiles=5)
    x, a, v, t = torch.zeros(4, 64), torch.zeros(4, 3), torch.zeros(4), torch.zeros(4, 9)
    for call in (lambda: head(x), lambda: head.action_log_prob(x), lambda: head.quantiles(x, a), lambda: head.quantiles(x, a, target=True),
                 lambda: head.td_target(x, v, v, 0.99, ent_coef=0.1), lambda: head.critic_loss(x, a, t), lambda: head.critic_loss(x, a, t, weights=v, return_td_errors=True),
                 lambda: head.actor_loss(x, ent_coef=0.1), lambda: head.polyak_update(0.005), lambda: head.ent_coef_loss(torch.zeros(1), v, -3.0),
                 lambda: TQ.critic_loss_from(torch.zeros(3, 4, 5), t), lambda: TQ.actor_loss_from(v, torch.zeros(3, 4, 5), 0.1)):
        with pytest.raises(m3l_amd.M3LError):
            call()


def test_other_heads_are_untouched():
    for n in (1, 3):
        with pytest.raises(ValueError, match="exactly 2 critics"):
            m3l_amd.SACHead(64, 3, n_critics=n)
    with pytest.raises(TypeError):
        m3l_amd.SACEnsembleHead(64, 3, n_quantiles=25)
    with pytest.raises(ValueError):          # a TQC head is no ensemble of one-output critics
        m3l_amd.sac._arch(64, m3l_amd.SACEnsembleParams.from_policy(TQCHead(64, 3, net_arch=[64], n_critics=2, n_quantiles=5)))


# ---- the restatement against a second version written with loops

def _loop_target(z_next, logp, r, done, gamma, ent, N, nq, d):
    B = z_next.shape[1]
    K = N * (nq - d)
    out = np.zeros((B, K))
    for b in range(B):
        pool = sorted(float(z_next[c, b, j]) for c in range(N) for j in range(nq))
        g = gamma if np.ndim(gamma) == 0 else gamma[b]
        for k in range(K):
            out[b, k] = r[b] + (1.0 - done[b]) * g * (pool[k] - ent * logp[b])
    return out


def _loop_loss(z, t, w):
    """loss, d loss / d z by the closed form of the header's rule 3, td_abs."""
    N, B, nq = z.shape
    K = t.shape[1]
    norm = B * N * nq * K
    loss, coef, td = 0.0, np.zeros_like(z), np.zeros(B)
    for b in range(B):
        for c in range(N):
            for j in range(nq):
                tau = (j + 0.5) / nq
                for k in range(K):
                    delta = t[b, k] - z[c, b, j]
                    huber = 0.5 * delta * delta if abs(delta) <= 1 else abs(delta) - 0.5
                    a = abs(tau - (1.0 if delta < 0 else 0.0))
                    loss += w[b] * a * huber
                    coef[c, b, j] -= w[b] / norm * a * min(max(delta, -1.0), 1.0)
                    td[b] += abs(delta) / (N * nq * K)
    return loss / norm, coef, td


@pytest.mark.parametrize("name", ["f16_a1_nohid_n1q1d0_b1", "f32_a7_q32_n2q25d2_b17", "f16_a7_q48x32_n3q5d4_b37", "f16_a1_q32_n3q5d4_b1", "f32_a7_q48x32_n5q7d3_b17"])
def test_restatement_against_the_loop_version(name):
    """torch.sort / [:, :K] / the 4-D broadcast / .mean() against plain loops, and autograd's gradient in z against the closed form, to 1e-12."""
    c, ref = TC.case(name), TC.reference(name)
    N, nq, d, ent = c["n_critics"], c["n_quantiles"], c["drop"], TC.ent_of(c)
    r, done = c["rewards"].astype(np.float64), c["dones"].astype(np.float64)
    close = lambda got, want: float(np.abs(np.asarray(got) - want).max()) <= 1e-12 * max(1.0, float(np.abs(want).max()))      # noqa: E731
    for gamma in (c["gamma"], c["discounts"].astype(np.float64)):
        want = _loop_target(ref["z_next"], ref["log_prob_next"], r, done, gamma, ent, N, nq, d)
        got = TC.target_ref(c, gamma, ent)
        assert got.shape == (r.size, c["K"]) and close(got, want), (name, "target")
        assert bool((np.diff(got[done == 0], axis=1) >= 0).all()), "kept quantiles ascend"
    target = TC.target_ref(c, c["gamma"], ent)
    for w in (None, c["weights"]):
        got = TC.critic_loss_ref(c, target, w)
        loss, coef, td = _loop_loss(ref["z_replay"], target, np.ones(r.size) if w is None else w.astype(np.float64))
        assert close(got["loss"], loss) and close(got["coef"], coef) and close(got["td_abs"], td), (name, "loss", w is None)
    al = TC.actor_loss_ref(c, ent)
    assert close(al["loss"], float(np.mean(ent * ref["log_prob"] - ref["z_pi"].mean(axis=(0, 2)))))


def test_hand_computed_example():
    """N = 1, nq = 2, K = 2 on one row: z = (0, 1), target = (0, 3).  delta: 0 - 0 = 0 (exactly), 3 - 0 = 3 (beyond 1), 0 - 1 = -1 (exactly
    -1), 3 - 1 = 2.  tau = (0.25, 0.75).
      j = 0: |0.25 - 0| 0 + |0.25 - 0| (3 - 0.5) = 0.625;       gradient sum: 0.25 * 0 + 0.25 * 1 = 0.25
      j = 1: |0.75 - 1| 0.5 (-1)^2 + |0.75 - 0| (2 - 0.5) = 0.125 + 1.125 = 1.25;       gradient sum: 0.25 * (-1) + 0.75 * 1 = 0.5
    loss = (0.625 + 1.25) / 4 = 0.46875;  d loss / d z = -(0.25, 0.5) / 4;  td = (0 + 3 + 1 + 2) / 4 = 1.5."""
    z = torch.tensor([[[0.0, 1.0]]], dtype=torch.float64, requires_grad=True)
    t = torch.tensor([[0.0, 3.0]], dtype=torch.float64)
    loss = TC.quantile_huber_loss(z, t)
    loss.backward()
    assert float(loss.detach()) == 0.46875 and z.grad.flatten().tolist() == [-0.0625, -0.125]
    l2, coef, td = _loop_loss(z.detach().numpy(), t.numpy(), np.ones(1))
    assert l2 == 0.46875 and coef.flatten().tolist() == [-0.0625, -0.125] and td.tolist() == [1.5]
    w = torch.tensor([2.0], dtype=torch.float64)
    assert float(TC.quantile_huber_loss(z.detach(), t, w)) == 0.9375
    # the sort / keep rule by hand: two nets of three quantiles, one dropped per net: the four smallest of the six, ascending
    zn = torch.tensor([[[3.0, -1.0, 2.0]], [[0.5, 4.0, -2.0]]], dtype=torch.float64)
    got = TC.truncated_target(zn, torch.tensor([1.0], dtype=torch.float64), torch.tensor([10.0], dtype=torch.float64), torch.tensor([0.0], dtype=torch.float64),
                              torch.tensor([0.5], dtype=torch.float64), 0.25, 4)
    assert got.tolist() == [[10 + 0.5 * (v - 0.25) for v in (-2.0, -1.0, 0.5, 2.0)]]
    done = TC.truncated_target(zn, torch.tensor([1.0], dtype=torch.float64), torch.tensor([10.0], dtype=torch.float64), torch.tensor([1.0], dtype=torch.float64),
                               torch.tensor([0.5], dtype=torch.float64), 0.25, 4)
    assert done.tolist() == [[10.0] * 4]


def test_case_table_reaches_the_grid():
    cases = list(TC.CASES.values())
    assert {c[6] for c in cases} == {1, 17, 37} and {c[0] for c in cases} == {16, 32} and {c[2] for c in cases} == {1, 7}
    assert {c[1] for c in cases} == {(), (32,), (48, 32)}
    assert {c[3:6] for c in cases} == {(1, 1, 0), (2, 25, 2), (3, 5, 4), (2, 64, 0), (5, 7, 3), (10, 25, 2)}
    assert all(c[6] == 17 for c in cases if c[3:6] in ((5, 7, 3), (10, 25, 2)))
    assert TC.CASES[TC.STEP][3:] == (2, 25, 2, 37) and TC.CASES[TC.ANCHOR][3:6] == (1, 1, 0)
    for name in TC.CASES:          # every (Huber branch, indicator side) occurs wherever the case has more than a handful of pairs
        c, ref = TC.case(name), TC.reference(name)
        t = TC.target_ref(c, c["gamma"], TC.ent_of(c))
        delta = t[:, None, None, :] - ref["z_replay"].transpose(1, 0, 2)[..., None]
        if delta.size >= 100:
            assert 0.05 < float((np.abs(delta) > 1).mean()) < 0.95 and 0.05 < float((delta < 0).mean()) < 0.95, name
