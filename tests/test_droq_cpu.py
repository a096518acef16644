"""CPU-only checks of the SAC DroQ critics: the C ABI declarations and descriptor packing, the public surface (SACEnsembleHead with
critic_layer_norm / critic_dropout: keys, refusals, seeds), the float64 restatement of tests/droq_cases.py (against sac_ens_cases with LayerNorm
off, and its LayerNorm + dropout backward against hand-derived formulas), and, for every case the GPU tests use, the conditions their
comparisons rest on.  No kernel is launched here."""
import ctypes as C
import os

import numpy as np
import pytest
import torch
from torch import nn

import droq_cases as DC
import m3l_amd
import sac_cases as SC
import sac_ens_cases as EC
from m3l_amd import _lib as L
from m3l_amd import sac as SH
from m3l_amd import sac_ensemble as SE
from test_dropout_cpu import dropout_mask, keep_scale

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ["m3l_sac_droq_ws_bytes", "m3l_sac_droq_critic_fwd", "m3l_sac_droq_critic_bwd", "m3l_sac_droq_td_target"]
VALUE_TOL = GRAD_TOL = 1e-4        # the GPU tests' bounds


def _head(arch, n, **kw):
    Fd, pi, qf, A = arch
    return m3l_amd.SACEnsembleHead(Fd, A, net_arch=dict(pi=list(pi), qf=list(qf)), n_critics=n, **kw)


def test_symbols_are_declared_bound_and_versioned():
    hdr = open(os.path.join(ROOT, "include", "m3l_amd.h")).read()
    for s in SYMBOLS:
        assert s + "(" in hdr and s in L.EXPORTS and hasattr(L.lib(), s), s
    assert "typedef struct m3l_sac_droq_desc" in hdr and "SAC DroQ critics (ABI 420)" in hdr
    section = hdr.split("(ABI 420)")[1].split("typedef struct")[0]
    for word in ("parity unpinned", "TQC", "rstd", "4 c + l", "OWN index", "m3l_op_dropout_mask", "d gamma", "never stored"):
        assert word in section, word
    lib = L.lib()
    assert lib.m3l_version() >= 420
    # the ensemble's descriptor in front, then the two tables, p and the seed
    assert [n for n, _ in L.SacDroqDesc._fields_] == ["ens", "ln_weight", "ln_bias", "dropout_p", "seed"]
    assert L.SacDroqDesc.ens.offset == 0 and L.SacDroqDesc.ln_weight.offset == C.sizeof(L.SacEnsDesc) == 768
    assert L.SacDroqDesc.ln_bias.offset == 768 + 240 and L.SacDroqDesc.dropout_p.offset == 1248 and L.SacDroqDesc.seed.offset == 1256
    assert C.sizeof(L.SacDroqDesc) == 1264
    d = L.SacDroqDesc()
    d.ens.features, d.ens.actions, d.ens.n_pi, d.ens.n_qf, d.ens.n_critics = 256, 7, 2, 2, 2
    for l in range(2):
        d.ens.pi_width[l] = d.ens.qf_width[l] = 256
    ens = lib.m3l_sac_ens_ws_bytes(C.byref(d.ens), 256)
    # on top of the ensemble's: xh and dy of 2 x 2 layers, and their rstd
    assert lib.m3l_sac_droq_ws_bytes(C.byref(d), 256) == ens + 4 * (8 * 256 * 256 + 4 * 256)
    for field, bad in (("n_critics", 0), ("n_critics", 11), ("features", 40)):
        keep = getattr(d.ens, field)
        setattr(d.ens, field, bad)
        assert lib.m3l_sac_droq_ws_bytes(C.byref(d), 256) == 256, (field, bad)
        setattr(d.ens, field, keep)
    for bad in (1.0, -0.1, 1.5, float("nan")):
        d.dropout_p = bad
        assert lib.m3l_sac_droq_ws_bytes(C.byref(d), 256) == 256, bad
        assert lib.m3l_sac_droq_critic_fwd(C.byref(d), 256, None, None, None, None, None) != 0 and "dropout_p" in L.last_error()


def test_descriptor_packing():
    arch = SC.ARCHS["mixed"]
    head = _head(arch, 5, critic_layer_norm=True, critic_dropout=0.1)
    p = head.params()
    named = dict(head.named_parameters())
    assert p.n_critics == 5 and p.layer_norm and p.dropout_p == 0.1 and p.drops == (True, True) and len(p) == 5
    names = DC.critic_names(arch, 5)
    lin = [n for n in names if int(n.split(".")[2]) % 4 == 0]
    ln = [n for n in names if int(n.split(".")[2]) % 4 == 2]
    assert [t.data_ptr() for t in p.critic_flat()] == [named[n].data_ptr() for n in lin]
    assert [t.data_ptr() for t in p.ln_flat()] == [named[n].data_ptr() for n in ln]
    assert [t.data_ptr() for t in p.ln_flat(True)] == [named[n.replace("critic.", "critic_target.")].data_ptr() for n in ln]
    a = SH._arch(arch[0], p)
    assert a == (32, 1, (32,), (64, 48, 16))
    d = SE._droq_desc(a, 5, 0.1, DC.SEED_Q, actor=p.actor_flat(), critic=p.critic_flat(True), ln=p.ln_flat(True))
    assert (d.ens.features, d.ens.actions, d.ens.n_qf, d.ens.n_critics, list(d.ens.qf_width)) == (32, 1, 3, 5, [64, 48, 16])
    assert d.dropout_p == np.float32(0.1) and d.seed == DC.SEED_Q
    for c in range(5):
        net = getattr(head.critic_target, f"qf{c}")
        assert [d.ens.qf_weight[c][l] for l in range(3)] == [net[4 * l].weight.data_ptr() for l in range(3)]
        assert [d.ln_weight[c][l] for l in range(3)] == [net[4 * l + 2].weight.data_ptr() for l in range(3)]
        assert [d.ln_bias[c][l] for l in range(3)] == [net[4 * l + 2].bias.data_ptr() for l in range(3)]
        assert d.ens.q_weight[c] == net[12].weight.data_ptr()
    assert d.ln_weight[5][0] is None and d.ln_bias[9][2] is None


@pytest.mark.parametrize("n,p", [(1, 0.0), (2, 0.01), (10, 0.5)])
def test_state_dict_keys_and_modules(n, p):
    """Linear at 4 l, Dropout at 4 l + 1 (present at p = 0 too), LayerNorm at 4 l + 2, ReLU at 4 l + 3, the output Linear at 4 n_qf; the keys do
    not depend on p; the target starts as a copy and takes no gradient; both sub-modules start in train mode."""
    arch = SC.ARCHS["mixed"]
    head = _head(arch, n, critic_layer_norm=True, critic_dropout=p)
    sd = head.state_dict()
    assert list(sd.keys()) == DC.param_names(arch, n)
    assert list(sd.keys()) == list(_head(arch, n, critic_layer_norm=True).state_dict().keys())
    for name in ("critic", "critic_target"):
        for c in range(n):
            net = getattr(getattr(head, name), f"qf{c}")
            assert [type(m) for m in net] == [nn.Linear, nn.Dropout, nn.LayerNorm, nn.ReLU] * 3 + [nn.Linear]
            assert all(net[4 * l + 1].p == p and net[4 * l + 2].eps == 1e-5 and net[4 * l + 2].normalized_shape == (w,) for l, w in enumerate(arch[2]))
            assert tuple(net[12].weight.shape) == (1, 16)
    for k in DC.critic_names(arch, n):
        assert torch.equal(sd[k], sd["critic_target." + k[len("critic."):]])
    assert [k for k, t in head.named_parameters() if t.requires_grad] == SC.actor_names(arch) + DC.critic_names(arch, n)
    assert head.critic.training and head.critic_target.training and head.last_dropout_seeds == {"q_values": None, "td_target": None}
    head.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in DC.make_inputs(arch, n, 2, p, 77)["params"].items()}, strict=True)


def test_defaults_leave_the_ensemble_head_as_it_is():
    arch = SC.ARCHS["mixed"]
    torch.manual_seed(3)
    a = _head(arch, 3)
    torch.manual_seed(3)
    b = _head(arch, 3, critic_layer_norm=False, critic_dropout=0.0)
    assert list(a.state_dict().keys()) == EC.param_names(arch, 3) == list(b.state_dict().keys())
    assert all(torch.equal(v, b.state_dict()[k]) for k, v in a.state_dict().items())
    p = a.params()
    assert not p.layer_norm and p.qf_ln == () and p.qf_target_ln == () and p.dropout_p == 0.0 and p.ln_flat() == []
    state = torch.get_rng_state()
    assert a._seed("q_values", p, False, None) is None and torch.equal(torch.get_rng_state(), state), "a head without dropout draws no seed"
    # no hidden critic layer: LayerNorm on has no site, and the head still says so
    p = _head(SC.ARCHS["amax"], 3, critic_layer_norm=True, critic_dropout=0.1).params()
    assert p.layer_norm and p.qf_ln == ((), (), ()) and p.dropout_p == 0.1
    assert list(_head(SC.ARCHS["amax"], 3, critic_layer_norm=True).state_dict().keys()) == EC.param_names(SC.ARCHS["amax"], 3)


def test_train_and_eval_rule_and_seeds():
    head = _head(SC.ARCHS["a64"], 2, critic_layer_norm=True, critic_dropout=0.01)
    p = head.params()
    assert p.active_dropout() == 0.01 and p.active_dropout(True) == 0.01
    head.critic_target.eval()
    p = head.params()
    assert p.drops == (True, False) and p.active_dropout() == 0.01 and p.active_dropout(True) == 0.0
    assert head._seed("td_target", p, True, 5) is None and head.last_dropout_seeds["td_target"] is None
    head.eval()
    assert head.params().drops == (False, False)
    head.train()
    p = head.params()
    torch.manual_seed(11)
    s1 = head._seed("q_values", p, False, None)
    torch.manual_seed(11)
    assert head._seed("q_values", p, False, None) == s1 == head.last_dropout_seeds["q_values"] and 0 <= s1 < 2 ** 63
    assert head._seed("td_target", p, True, 123) == 123 == head.last_dropout_seeds["td_target"] and head.last_dropout_seeds["q_values"] == s1
    for bad in (-1, 2 ** 64, 1.5, "7", True):
        with pytest.raises(ValueError, match="dropout_seed"):
            head._seed("q_values", p, False, bad)
    # p = 0: LayerNorm critics never draw
    plain = _head(SC.ARCHS["a64"], 2, critic_layer_norm=True)
    state = torch.get_rng_state()
    assert plain._seed("q_values", plain.params(), False, None) is None and torch.equal(torch.get_rng_state(), state)


def test_every_refusal_that_needs_no_device():
    H = m3l_amd.SACEnsembleHead
    for bad in (1.0, -0.01, 1.5, "0.1", None, True, float("nan")):
        with pytest.raises(ValueError, match="critic_dropout"):
            H(64, 3, n_critics=2, critic_layer_norm=True, critic_dropout=bad)
    for p in (0.01, 0.5):
        with pytest.raises(ValueError, match="critic_layer_norm=True"):
            H(64, 3, n_critics=2, critic_dropout=p)
    for bad in (1, "yes", None):
        with pytest.raises(ValueError, match="critic_layer_norm"):
            H(64, 3, n_critics=2, critic_layer_norm=bad)
    for n in (1, 3):          # SACHead is untouched
        with pytest.raises(ValueError, match="exactly 2 critics"):
            m3l_amd.SACHead(64, 3, n_critics=n)
    with pytest.raises(TypeError):
        m3l_amd.SACHead(64, 3, critic_layer_norm=True)
    # CPU tensors raise: nothing falls back
    head = H(64, 3, net_arch=dict(pi=[64], qf=[64]), n_critics=2, critic_layer_norm=True, critic_dropout=0.1)
    x, a, v = torch.zeros(4, 64), torch.zeros(4, 3), torch.zeros(4)
    for call in (lambda: head.q_values(x, a), lambda: head.q_values(x, a, dropout_seed=3), lambda: head.td_target(x, v, v, 0.99, ent_coef=0.1, dropout_seed=3),
                 lambda: head.critic_loss(x, a, v, dropout_seed=3), lambda: head.actor_loss(x, ent_coef=0.1, dropout_seed=3), lambda: head.polyak_update(0.005)):
        with pytest.raises(m3l_amd.M3LError):
            call()


def test_from_policy_on_mismatching_layouts():
    arch = SC.ARCHS["a64"]
    FP = SE.SACEnsembleParams.from_policy

    def droq(**kw):
        return _head(arch, 3, critic_layer_norm=True, critic_dropout=0.1, **kw)
    plain = _head(arch, 3)
    m = droq()
    m.critic.qf1 = plain.critic.qf1          # one critic without LayerNorm
    with pytest.raises(ValueError, match="one layout"):
        FP(m)
    m = droq()
    m.critic_target = plain.critic_target          # the targets without LayerNorm
    with pytest.raises(ValueError, match="one layout"):
        FP(m)
    m = _head(arch, 3)
    m.critic.qf0 = droq().critic.qf0          # a LayerNorm net in a head that says it has none
    with pytest.raises(ValueError, match="one layout"):
        FP(m)
    m = droq()
    m.critic.qf2[1] = nn.Dropout(0.2)
    with pytest.raises(ValueError, match="one rate"):
        FP(m)
    m = droq()
    m.critic_target.qf0[5].p = 0.3
    with pytest.raises(ValueError, match="one rate"):
        FP(m)
    m = droq()
    m.critic.qf1[1].eval()
    with pytest.raises(ValueError, match="train mode and some in eval mode"):
        FP(m)
    m = droq()
    m.critic.qf0[2] = nn.LayerNorm(64, eps=1e-6)
    with pytest.raises(ValueError, match="eps 1e-5"):
        FP(m)
    m = droq()
    m.critic.qf0[2] = nn.LayerNorm(64, elementwise_affine=False)
    with pytest.raises(ValueError, match="elementwise affine"):
        FP(m)
    m = droq()
    m.critic.qf0[1], m.critic.qf0[2] = m.critic.qf0[2], m.critic.qf0[1]          # LayerNorm in front of Dropout
    with pytest.raises(ValueError, match="nn.Dropout expected"):
        FP(m)
    m = droq()
    m.critic.qf0[3] = nn.Tanh()
    with pytest.raises(ValueError, match="ReLU only"):
        FP(m)
    m = droq()
    m.critic.qf2 = _head((64, (64,), (64, 32), 3), 1, critic_layer_norm=True, critic_dropout=0.1).critic.qf0          # other widths
    with pytest.raises(ValueError, match="must be alike"):
        SH._arch(64, FP(m))
    # a module without the head's attributes, with SB3's names, is read from its layers alone
    bare = nn.Module()
    bare.actor, bare.critic, bare.critic_target = droq().actor, nn.Module(), nn.Module()
    src = droq()
    for i in range(3):
        setattr(bare.critic, f"qf{i}", getattr(src.critic, f"qf{i}"))
        setattr(bare.critic_target, f"qf{i}", getattr(src.critic_target, f"qf{i}"))
    p = FP(bare)
    assert p.layer_norm and p.dropout_p == 0.1 and p.drops == (True, True) and len(p.ln_flat()) == 12


def test_case_table():
    assert set(DC.CASES.values()) == {("aligned", 2, 1, 0.25), ("mixed", 3, 33, 0.1), ("a64", 2, 17, 0.01), ("a64", 2, 33, 0.0), ("a64", 10, 33, 0.5),
                                      ("amax", 3, 3, 0.1), ("w512", 1, 17, 0.1)}
    assert DC.CASES[DC.ANCHOR] == ("a64", 2, 17, 0.01) and DC.ARCHS["w512"] == (64, (64,), (512,), 3) and [9, 0] in EC.subsets(10)
    assert 0 < DC.SEED_Q < 2 ** 63 and 0 < DC.SEED_T < 2 ** 63 and DC.SEED_Q != DC.SEED_T


def test_restatement_without_layer_norm_is_sac_ens_cases():
    """LayerNorm off and no masks: critic_forward is sac_ens_cases.critic_forward, in every bit of q and of every gate quantity."""
    for name in ("a64_n2_b33", "mixed_n3_b33", "amax_n3_b17"):
        c = EC.case(name)
        P = SC.as_torch(c["params"])
        x, a = torch.from_numpy(c["x"]).double(), torch.from_numpy(c["a_replay"]).double()
        for prefix in ("critic", "critic_target"):
            q0, pre0 = EC.critic_forward(P, prefix, x, a, c["n_critics"])
            q1, pre1 = DC.critic_forward(P, prefix, x, a, c["n_critics"], layer_norm=False)
            assert torch.equal(q0, q1) and len(pre0) == len(pre1) and all(torch.equal(u, v) for u, v in zip(pre0, pre1)), (name, prefix)


def test_restatement_uses_the_contract_masks_by_the_critics_own_index():
    """The mask of site (c, l) is dropout_mask(p, seed, c, l, B, w); a critic evaluated alone keeps the masks of its index."""
    c = DC.case("a64_n10_b33_p50")
    m = DC.masks_of(c, DC.SEED_Q)
    assert set(m) == {(ci, l) for ci in range(10) for l in range(2)}
    assert np.array_equal(m[(9, 1)].numpy(), dropout_mask(0.5, DC.SEED_Q, 9, 1, 33, 64)) and not torch.equal(m[(9, 1)], m[(0, 1)])
    assert DC.masks_of(c, None) is None and DC.masks_of(DC.case("a64_n2_b33_p0"), DC.SEED_Q) is None
    assert c["scale"] == keep_scale(0.5) == 2.0 and DC.case("a64_n2_b33_p0")["scale"] == 1.0
    ref = DC.reference("a64_n10_b33_p50")
    P = SC.as_torch(c["params"])
    one = {k.replace(".qf9.", ".qf0."): v for k, v in P.items() if ".qf9." in k}
    q, _ = DC.critic_forward(one, "critic_target", torch.from_numpy(c["x_next"]).double(), torch.from_numpy(ref["a_next"]),
                             1, {(0, l): DC.masks_of(c, DC.SEED_T)[(9, l)] for l in range(2)}, c["scale"])
    assert np.array_equal(q.detach().numpy()[0], ref["q_next"][9])


def test_hand_derived_backward_against_autograd():
    """The header's LayerNorm + dropout backward in float64 against autograd of the restatement's forward, to 1e-12."""
    g = torch.Generator().manual_seed(5)
    rn = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)      # noqa: E731
    for B, w, p in ((5, 48, 0.3), (3, 16, 0.0), (7, 512, 0.1)):
        z = rn(B, w).requires_grad_(True)
        gamma, beta = (1 + 0.2 * rn(w)).requires_grad_(True), (0.2 * rn(w)).requires_grad_(True)
        keep = torch.from_numpy(dropout_mask(p, 99, 1, 2, B, w)).double() if p > 0 else torch.ones(B, w, dtype=torch.float64)
        scale = keep_scale(p) if p > 0 else 1.0
        h = torch.relu(torch.nn.functional.layer_norm(z * keep * scale, (w,), gamma, beta, 1e-5))
        gh = rn(B, w)
        (h * gh).sum().backward()
        with torch.no_grad():
            d = z * keep * scale
            mean = d.sum(1, keepdim=True) / w
            var = ((d - mean) ** 2).sum(1, keepdim=True) / w
            rstd = 1 / torch.sqrt(var + 1e-5)
            xh = (d - mean) * rstd
            hh = torch.clamp(xh * gamma + beta, min=0)
            dy = gh * (hh > 0)
            dgamma, dbeta = (dy * xh).sum(0), dy.sum(0)
            dxh = dy * gamma
            dd = rstd * (dxh - dxh.mean(1, keepdim=True) - xh * (dxh * xh).mean(1, keepdim=True))
            dz = dd * keep * scale
        for what, got, want in (("h", hh, h), ("dz", dz, z.grad), ("dgamma", dgamma, gamma.grad), ("dbeta", dbeta, beta.grad)):
            assert float((got - want.detach()).abs().max()) <= 1e-12 * max(1.0, float(want.detach().abs().max())), (B, w, p, what)


def _rel(got, ref):
    return float((np.abs(got - ref) / np.maximum(1.0, np.abs(ref))).max())


def _grad_err(got, ref):
    assert set(got) == set(ref)
    worst = 0.0
    for k, r in ref.items():
        gmax = float(np.abs(r).max())
        worst = max(worst, float(np.abs(got[k] - r).max()) / gmax if gmax > 0 else float(np.abs(got[k]).max()))
    return worst


@pytest.mark.parametrize("name", list(DC.CASES))
def test_input_conditions_and_float32_restatement(name):
    """What the GPU comparisons rest on: gate, tie and clamp margins in float64 over every evaluation; the float32 restatement has the same gates
    and the same chosen critics, and every quantity the GPU tests check, values and gradients, stays within a quarter of its bound."""
    c, ref = DC.case(name), DC.reference(name)
    arch, N, B, p = c["arch"], c["n_critics"], c["x"].shape[0], c["dropout_p"]
    assert list(c["params"]) == DC.param_names(arch, N) and all(ref[k].shape == (N, B) for k in DC.EVALS)
    assert len(ref["pre"]) == len(DC._pre_owner(arch, N)) == 2 * len(arch[1]) + 6 * N * len(arch[2])
    cond = DC.conditions(ref, N)
    assert cond["gate"] >= SC.GATE_MARGIN and cond["tie"] >= SC.TIE_MARGIN and cond["clamp"] >= SC.CLAMP_MARGIN, (name, cond)
    if p > 0 and arch[2]:          # the masks matter: train and eval mode differ, and some element of every site is dropped
        assert not np.array_equal(ref["q_replay"], ref["q_replay_eval"]) and not np.array_equal(ref["q_next"], ref["q_next_eval"])
        assert all(not bool(m.all()) or B * m.shape[1] * p < 1 for m in DC.masks_of(c, DC.SEED_Q).values())
    else:
        assert np.array_equal(ref["q_replay"], ref["q_replay_eval"]) and np.array_equal(ref["q_next"], ref["q_next_eval"])
    f32 = DC.forward_ref(c, torch.float32)
    for a, b in zip(f32["pre"], ref["pre"]):
        assert np.array_equal(a > 0, b > 0), (name, "a float32 gate differs from the float64 gate")
    assert np.array_equal(f32["q_pi"].argmin(axis=0), ref["q_pi"].argmin(axis=0)), name
    for key in ("q_next", "q_next_eval"):
        for sub in EC.subsets(N)[1:]:
            assert np.array_equal(f32[key][sub].argmin(axis=0), ref[key][sub].argmin(axis=0)), (name, key, sub)
    worst = {}
    for k in DC.EVALS + ("a_pi", "log_prob", "log_prob_next"):
        worst[k] = _rel(f32[k], ref[k])
    ent = EC.ent_of(c)
    dq = torch.randn(N, B, generator=torch.Generator().manual_seed(11)).numpy()
    for what, kw in (("q_ref", {}), ("q_ref eval", dict(seed=None)), ("q_ref target", dict(prefix="critic_target"))):
        r64, r32 = DC.q_ref(c, c["a_replay"], dq, **kw), DC.q_ref(c, c["a_replay"], dq, dtype=torch.float32, **kw)
        worst[what] = max(_rel(r32["q"], r64["q"]), _grad_err(r32["grad"], r64["grad"]))
    target = DC.target_ref(c, ref, None, c["gamma"], ent)
    for what, w in (("critic_loss", None), ("critic_loss weighted", c["weights"])):
        r64, r32 = DC.critic_loss_ref(c, target, w), DC.critic_loss_ref(c, target, w, dtype=torch.float32)
        worst[what] = max(_rel(r32["loss"], r64["loss"]), _rel(r32["td_abs"], r64["td_abs"]), _grad_err(r32["grad"], r64["grad"]))
    for reduce in ("min", "mean"):
        r64, r32 = DC.actor_loss_ref(c, reduce, ent), DC.actor_loss_ref(c, reduce, ent, dtype=torch.float32)
        worst["actor_loss " + reduce] = max(_rel(r32["loss"], r64["loss"]), _grad_err(r32["grad"], r64["grad"]))
    print(f"[{name}] float32 restatement against float64: " + ", ".join(f"{k} {v:.1e}" for k, v in worst.items()))
    assert max(worst.values()) <= VALUE_TOL / 4, (name, worst)
    assert float(c["weights"].min()) >= 0.25 and (len(set(c["discounts"].tolist())) > 1 or B == 1)
