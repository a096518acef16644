"""CPU-only checks of the SAC critic ensemble: the C ABI declarations and descriptor packing, the public surface (SACEnsembleHead: SB3's names for
N critics, every refusal that needs no device), the float64 restatement of tests/sac_ens_cases.py against sac_cases' own step at N = 2, and, for
every case the GPU tests use, the conditions their comparisons rest on.  No kernel is launched here."""
import ctypes as C
import os

import numpy as np
import pytest
import torch
from torch import nn

import m3l_amd
import sac_cases as SC
import sac_ens_cases as EC
from m3l_amd import _lib as L
from m3l_amd import sac as SH
from m3l_amd import sac_ensemble as SE

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ["m3l_sac_ens_ws_bytes", "m3l_sac_ens_critic_fwd", "m3l_sac_ens_critic_bwd", "m3l_sac_ens_td_target", "m3l_sac_ens_critic_loss_fwd",
           "m3l_sac_ens_actor_loss_fwd", "m3l_sac_ens_loss_bwd"]
VALUE_TOL = GRAD_TOL = 1e-4        # the GPU tests' bounds


def test_symbols_are_declared_bound_and_versioned():
    hdr = open(os.path.join(ROOT, "include", "m3l_amd.h")).read()
    for s in SYMBOLS:
        assert s + "(" in hdr and s in L.EXPORTS and hasattr(L.lib(), s), s
    assert "typedef struct m3l_sac_ens_desc" in hdr and "M3L_SAC_MAX_CRITICS 10" in hdr and "SAC critic ensemble (ABI 419)" in hdr
    section = hdr.split("(ABI 419)")[1].split("/* ----")[0]
    for word in ("parity unpinned", "DroQ", "TQC", "NaN", "lowest index"):
        assert word in section, word
    lib = L.lib()
    assert lib.m3l_version() >= 419 and L.SAC_MAX_CRITICS == SE.MAX_CRITICS == EC.MAX_CRITICS == 10
    d = L.SacEnsDesc()
    d.features, d.actions, d.n_pi, d.n_qf, d.n_critics = 256, 7, 2, 2, 10
    for l in range(2):
        d.pi_width[l] = d.qf_width[l] = 256
    # at least: 10 x 2 hidden activations and their gradients, the critics' input and d q
    assert lib.m3l_sac_ens_ws_bytes(C.byref(d), 256) >= 4 * (40 * 256 * 256 + 256 * 263 + 10 * 256)
    for field, bad in (("n_critics", 0), ("n_critics", 11), ("features", 40), ("actions", 65)):
        keep = getattr(d, field)
        setattr(d, field, bad)
        assert lib.m3l_sac_ens_ws_bytes(C.byref(d), 256) == 256, (field, bad)          # an unsupported shape sizes nothing
        setattr(d, field, keep)


def test_descriptor_packing():
    """Field order and sizes of the ctypes mirror against the header's struct, and the pointers of a head in their slots."""
    assert [n for n, _ in L.SacEnsDesc._fields_] == [n for n, _ in L.SacDesc._fields_[:12]] + ["n_critics", "qf_weight", "qf_bias", "q_weight", "q_bias"]
    # the actor's part lies as in m3l_sac_desc; n_critics and its padding, then the four tables of 10
    assert all(getattr(L.SacEnsDesc, n).offset == getattr(L.SacDesc, n).offset for n, _ in L.SacDesc._fields_[:12])
    assert L.SacEnsDesc.n_critics.offset == 120 and L.SacEnsDesc.qf_weight.offset == 128 and C.sizeof(L.SacEnsDesc) == 128 + (30 + 30 + 10 + 10) * 8
    arch = SC.ARCHS["mixed"]
    head = m3l_amd.SACEnsembleHead(arch[0], arch[3], net_arch=dict(pi=list(arch[1]), qf=list(arch[2])), n_critics=5)
    p = head.params()
    named = dict(head.named_parameters())
    assert p.n_critics == 5
    assert [t.data_ptr() for t in p.actor_flat()] == [named[n].data_ptr() for n in SC.actor_names(arch)]
    assert [t.data_ptr() for t in p.critic_flat()] == [named[n].data_ptr() for n in EC.critic_names(arch, 5)]
    assert [t.data_ptr() for t in p.critic_flat(True)] == [named[n].data_ptr() for n in EC.critic_names(arch, 5, "critic_target")]
    a = SH._arch(arch[0], p)
    assert a == (32, 1, (32,), (64, 48, 16))
    d = SE._ens_desc(a, 5, actor=p.actor_flat(), critic=p.critic_flat(True))
    assert (d.features, d.actions, d.n_pi, d.n_qf, d.n_critics, list(d.qf_width)) == (32, 1, 1, 3, 5, [64, 48, 16])
    assert d.mu_weight == head.actor.mu.weight.data_ptr() and d.log_std_bias == head.actor.log_std.bias.data_ptr()
    for c in range(5):
        net = getattr(head.critic_target, f"qf{c}")
        assert [d.qf_weight[c][l] for l in range(3)] == [net[2 * l].weight.data_ptr() for l in range(3)]
        assert [d.qf_bias[c][l] for l in range(3)] == [net[2 * l].bias.data_ptr() for l in range(3)]
        assert d.q_weight[c] == net[6].weight.data_ptr() and d.q_bias[c] == net[6].bias.data_ptr()
    assert d.q_weight[5] is None and d.qf_weight[9][0] is None


def _sb3_like(features_dim, action_dim, pi, qf, n):
    """A hand-built policy with SB3's names behind the extractor and n critics, in the creation order of SB3 2.x's SACPolicy._build."""
    def seq(k, widths, out=None):
        mods = []
        for w in widths:
            mods += [nn.Linear(k, w), nn.ReLU()]
            k = w
        if out is not None:
            mods.append(nn.Linear(k, out))
        return nn.Sequential(*mods), k
    m = nn.Module()
    m.actor = nn.Module()
    m.actor.latent_pi, k = seq(features_dim, pi)
    m.actor.mu = nn.Linear(k, action_dim)
    m.actor.log_std = nn.Linear(k, action_dim)
    for name in ("critic", "critic_target"):
        c = nn.Module()
        for i in range(n):
            setattr(c, f"qf{i}", seq(features_dim + action_dim, qf, 1)[0])
        setattr(m, name, c)
    return m


@pytest.mark.parametrize("n", [1, 3, 10])
def test_head_has_sb3_names_and_loads_strictly(n):
    Fd, pi, qf, A = arch = SC.ARCHS["mixed"]
    head = m3l_amd.SACEnsembleHead(Fd, A, net_arch=dict(pi=list(pi), qf=list(qf)), n_critics=n)
    ref = _sb3_like(Fd, A, pi, qf, n)
    sd, rd = head.state_dict(), ref.state_dict()
    assert list(sd.keys()) == list(rd.keys()) == EC.param_names(arch, n)
    assert [tuple(v.shape) for v in sd.values()] == [tuple(v.shape) for v in rd.values()]
    for k in EC.critic_names(arch, n):          # the target starts as a copy of the critic and takes no gradient
        assert torch.equal(sd[k], sd["critic_target." + k[len("critic."):]])
    assert [k for k, p in head.named_parameters() if p.requires_grad] == SC.actor_names(arch) + EC.critic_names(arch, n)
    head.load_state_dict(rd, strict=True)
    assert "SACEnsembleHead" in m3l_amd.__all__ and "SACEnsembleParams" in m3l_amd.__all__
    p = SE.SACEnsembleParams.from_policy(ref)          # an SB3-like object is read the same way
    assert p.n_critics == n
    assert [tuple(t.shape) for t in p.actor_flat() + p.critic_flat() + p.critic_flat(True)] == [tuple(v.shape) for v in rd.values()]


def test_default_architecture():
    head = m3l_amd.SACEnsembleHead(256, 7)
    assert head.n_critics == 10 and hasattr(head.critic, "qf9") and not hasattr(head.critic, "qf10")
    assert [tuple(p.shape) for p in head.critic.qf9.parameters()] == [(256, 263), (256,), (256, 256), (256,), (1, 256), (1,)]


def test_every_refusal_that_needs_no_device():
    H = m3l_amd.SACEnsembleHead
    for bad in (0, 11, -1, 2.5, 2.0, "3", True, None):
        with pytest.raises(ValueError, match="from 1 to 10"):
            H(64, 3, n_critics=bad)
    # SACHead's refusals, by its helpers
    for kw, why in ((dict(features_dim=40), "multiples of 16"), (dict(net_arch=dict(pi=[64], qf=[1024])), "at most 512"), (dict(action_dim=65), "1 to 64"),
                    (dict(net_arch=dict(pi=[16], qf=[16] * 4)), "0 to 3 hidden layers"), (dict(activation_fn=nn.Tanh), "ReLU only"),
                    (dict(use_sde=True), "use_sde"), (dict(share_features_extractor=False), "share_features_extractor=False")):
        args = dict(features_dim=64, action_dim=3, n_critics=3)
        args.update(kw)
        with pytest.raises(ValueError, match=why):
            H(**args)
    # critics that differ in widths
    m = _sb3_like(64, 3, (64,), (64,), 3)
    m.critic.qf2 = _sb3_like(64, 3, (64,), (32,), 1).critic.qf0
    with pytest.raises(ValueError, match="must be alike"):
        SH._arch(64, SE.SACEnsembleParams.from_policy(m))
    m = _sb3_like(64, 3, (64,), (64,), 3)
    del m.critic_target.qf2
    with pytest.raises(ValueError, match="must agree"):
        SE.SACEnsembleParams.from_policy(m)
    m = _sb3_like(64, 3, (64,), (64,), 11)
    with pytest.raises(ValueError, match="from 1 to 10"):
        SE.SACEnsembleParams.from_policy(m)
    m = _sb3_like(64, 3, (64,), (64,), 3)
    m.n_critics = 4
    with pytest.raises(ValueError, match="must agree"):
        SE.SACEnsembleParams.from_policy(m)
    m = _sb3_like(64, 3, (64,), (64,), 3)
    m.actor.latent_pi[1] = nn.Tanh()
    with pytest.raises(ValueError, match="ReLU only"):
        SE.SACEnsembleParams.from_policy(m)
    m = _sb3_like(64, 3, (64,), (64,), 3)
    m.actor.use_sde = True
    with pytest.raises(ValueError, match="use_sde"):
        SE.SACEnsembleParams.from_policy(m)
    # q_reduce and subset: refused for their form before any tensor is looked at
    head = H(64, 3, net_arch=dict(pi=[64], qf=[64]), n_critics=3)
    x, v = torch.zeros(4, 64), torch.zeros(4)
    for bad in ("max", "Min", None, 0):
        with pytest.raises(ValueError, match="q_reduce"):
            head.actor_loss(x, ent_coef=0.1, q_reduce=bad)
        with pytest.raises(ValueError, match="q_reduce"):
            SE.actor_loss_from(v, torch.zeros(3, 4), ent_coef=0.1, q_reduce=bad)
    i32 = torch.int32
    for bad in (torch.zeros(2, dtype=torch.int64), torch.zeros(2), torch.zeros(4, dtype=i32), torch.zeros(0, dtype=i32), torch.zeros(1, 2, dtype=i32),
                torch.zeros(4, dtype=i32)[::2], [0, 1], 1):
        with pytest.raises(ValueError, match="subset"):
            head.td_target(x, v, v, 0.99, ent_coef=0.1, subset=bad)
    for bad in (0, 4, 1.5, True):
        with pytest.raises(ValueError, match="sample_subset"):
            head.sample_subset(bad)
    s = head.sample_subset(2)
    assert s.dtype == i32 and s.shape == (2,) and s.is_contiguous() and len(set(s.tolist())) == 2 and set(s.tolist()) <= {0, 1, 2}


def test_cpu_tensors_raise_and_nothing_falls_back():
    head = m3l_amd.SACEnsembleHead(64, 3, net_arch=dict(pi=[64], qf=[64]), n_critics=3)
    x, a, v = torch.zeros(4, 64), torch.zeros(4, 3), torch.zeros(4)
    for call in (lambda: head(x), lambda: head.action_log_prob(x), lambda: head.q_values(x, a), lambda: head.td_target(x, v, v, 0.99, ent_coef=0.1),
                 lambda: head.td_target(x, v, v, 0.99, ent_coef=0.1, subset=torch.zeros(2, dtype=torch.int32)), lambda: head.critic_loss(x, a, v),
                 lambda: head.actor_loss(x, ent_coef=0.1, q_reduce="mean"), lambda: head.polyak_update(0.005),
                 lambda: SE.critic_loss_from(torch.zeros(3, 4), v), lambda: SE.actor_loss_from(v, torch.zeros(3, 4), 0.1)):
        with pytest.raises(m3l_amd.M3LError):
            call()


def test_sac_head_still_refuses_other_critic_counts():
    for n in (1, 3, 10):
        with pytest.raises(ValueError, match="exactly 2 critics"):
            m3l_amd.SACHead(64, 3, n_critics=n)
    with pytest.raises(ValueError, match="exactly 2 critics"):
        SH.SACHeadParams.from_policy(m3l_amd.SACEnsembleHead(64, 3, net_arch=[64], n_critics=3))
    with pytest.raises(ValueError, match="exactly 2 critics"):
        SH._arch(64, SH.SACHeadParams(*SE.SACEnsembleParams.from_policy(m3l_amd.SACEnsembleHead(64, 3, net_arch=[64], n_critics=3))))


def test_case_table_and_subsets():
    assert {(a, n, b) for a, n, b in EC.CASES.values()} == {("a64", 1, 17), ("a64", 2, 33), ("a64", 3, 17), ("a64", 10, 33), ("mixed", 3, 33),
                                                             ("mixed", 5, 1), ("nohid", 10, 3), ("amax", 3, 17)}
    assert EC.CASES[EC.ANCHOR] == ("a64", 2, 33)
    assert EC.subsets(1) == [None, [0], [0]]
    for n in (2, 3, 5, 10):
        s = EC.subsets(n)
        assert s[:3] == [None, [0], [n - 1]] and s[3][0] > s[3][1] and any(len(set(x)) < len(x) for x in s[4:])
        assert all(1 <= len(x) <= n and all(0 <= i < n for i in x) for x in s[1:])


def test_restatement_at_two_critics_is_sac_cases_step():
    """N = 2, subset None, the min reduction, unweighted: sac_cases.step_ref's values and gradients, in float64."""
    c = EC.case(EC.ANCHOR)
    ref = EC.reference(EC.ANCHOR)
    own = SC.step_ref(c)
    ent = float(own["ent_coef"])

    def close(what, got, want):
        got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
        assert got.shape == want.shape and float(np.abs(got - want).max()) <= 1e-12 * max(1.0, float(np.abs(want).max())), what
    for k in ("a_pi", "log_prob", "q_replay", "q_pi", "q_next", "a_next", "log_prob_next"):
        close(k, ref[k], own[k])
    target = EC.target_ref(c, ref, None, c["gamma"], ent)
    close("target_q", target, own["target_q"])
    cl = EC.critic_loss_ref(c, target)
    close("critic_loss", cl["loss"], own["critic_loss"])
    close("critic_loss with weights of ones", EC.critic_loss_ref(c, target, np.ones_like(c["weights"]))["loss"], own["critic_loss"])
    al = EC.actor_loss_ref(c, "min", ent)
    close("actor_loss", al["loss"], own["actor_loss"])
    for k, g in list(cl["grad"].items()) + list(al["grad"].items()):
        close("grad " + k, g, own["grad"][k])
    for k, v in EC.polyak_ref(c).items():
        close("target " + k, v, own["target"][k])
    # the pieces of the rule that sac_cases has no word for
    close("td_abs", cl["td_abs"], 0.5 * (np.abs(ref["q_replay"][0] - target) + np.abs(ref["q_replay"][1] - target)))
    close("coef", cl["coef"], (ref["q_replay"] - target) / target.size)
    mean = EC.actor_loss_ref(c, "mean", ent)
    close("actor_loss (mean)", mean["loss"], (ent * ref["log_prob"] - ref["q_pi"].mean(axis=0)).mean())
    close("one critic's target", EC.target_ref(c, ref, [1], c["gamma"], ent),
          c["rewards"].astype(np.float64) + (1.0 - c["dones"].astype(np.float64)) * c["gamma"] * (ref["q_next"][1] - ent * ref["log_prob_next"]))


def test_input_conditions_of_every_gpu_case():
    """What the GPU comparisons rest on: gate, tie and clamp margins in float64 for all N critics at every evaluation point and for every subset;
    the float32 restatement has the same gates and the same chosen critics and stays within a quarter of each bound; its pre-activation error
    is measured and stays under sac_cases.MEASURED_PRE_ERR, an eighth of the margin at most."""
    assert SC.GATE_MARGIN >= 8 * SC.MEASURED_PRE_ERR
    worst_pre = 0.0
    for name in EC.CASES:
        c, ref = EC.case(name), EC.reference(name)
        N = c["n_critics"]
        assert list(c["params"]) == EC.param_names(c["arch"], N) and ref["q_next"].shape == ref["q_pi"].shape == (N, c["x"].shape[0])
        cond = EC.conditions(ref, N)
        assert cond["gate"] >= SC.GATE_MARGIN and cond["tie"] >= SC.TIE_MARGIN and cond["clamp"] >= SC.CLAMP_MARGIN, (name, cond)
        if N >= 2:
            assert len(EC.tie_gaps(ref, N)) >= 3, name
        f32 = EC.forward_ref(c, torch.float32)
        assert len(f32["pre"]) == len(ref["pre"]) == len(EC._pre_owner(c["arch"], N))
        for a, b in zip(f32["pre"], ref["pre"]):
            assert np.array_equal(a > 0, b > 0), (name, "a float32 gate differs from the float64 gate")
            worst_pre = max(worst_pre, float(np.abs(a - b).max()))
        assert np.array_equal(f32["q_pi"].argmin(axis=0), ref["q_pi"].argmin(axis=0)), name
        for sub in EC.subsets(N)[1:]:
            assert np.array_equal(f32["q_next"][sub].argmin(axis=0), ref["q_next"][sub].argmin(axis=0)), (name, sub)
        for k in ("a_pi", "log_prob", "q_next", "q_replay", "q_pi", "log_prob_next"):
            err = float((np.abs(f32[k] - ref[k]) / np.maximum(1.0, np.abs(ref[k]))).max())
            assert err <= VALUE_TOL / 4, (name, k, err)
        assert float(c["weights"].min()) >= 0.25 and (len(set(c["discounts"].tolist())) > 1 or c["x"].shape[0] == 1)
    print(f"largest float32 pre-activation error over the ensemble cases: {worst_pre:.2e} (MEASURED_PRE_ERR {SC.MEASURED_PRE_ERR:.0e})")
    assert worst_pre <= SC.MEASURED_PRE_ERR, worst_pre
