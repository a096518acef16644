"""CPU-only checks of the SAC policy head: the C ABI declarations and descriptor packing, the public surface (SACHead: SB3's names and layouts,
every refusal with its reason), the float64 restatement of tests/sac_cases.py against torch.distributions.Normal, against the header's closed
forms and against the step recorded from the reference's own `SAC_MAE.train` (golden/sac_head_step.npz, golden/make_golden_sac_head.py), and,
for every case the GPU tests use, the conditions their comparisons rest on.  No kernel is launched here."""
import ctypes as C
import os
from functools import lru_cache

import numpy as np
import pytest
import torch
from torch import nn

import m3l_amd
import sac_cases as SC
from m3l_amd import _lib as L
from m3l_amd import sac as SH

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ["m3l_sac_ws_bytes", "m3l_sac_actor_fwd", "m3l_sac_actor_bwd", "m3l_sac_critic_fwd", "m3l_sac_critic_bwd", "m3l_sac_td_target",
           "m3l_sac_critic_loss_fwd", "m3l_sac_critic_loss_bwd", "m3l_sac_actor_loss_fwd", "m3l_sac_actor_loss_bwd", "m3l_sac_ent_coef_loss"]
GOLDEN_CASES = ["auto", "fixed", "clamped", "b1"]
VALUE_TOL = GRAD_TOL = 1e-4        # the GPU tests' bounds: 1e-4 max(1, |ref|); 1e-4 of a gradient's largest entry
INPUTS = ("x", "x_next", "noise_pi", "noise_next", "a_replay", "rewards", "dones")


@lru_cache(maxsize=None)
def _z():
    return np.load(os.path.join(ROOT, "tests", "golden", "sac_head_step.npz"))


@lru_cache(maxsize=None)
def golden_case(name):
    """(case in the form of sac_cases.make_inputs, recorded results) of a case of sac_head_step.npz."""
    z = _z()
    fl = z[f"{name}/flags"]
    c = {k: z[f"{name}/in/{k}"] for k in INPUTS}
    c["params"] = {k[len(f"{name}/param/"):]: z[k] for k in z.files if k.startswith(f"{name}/param/")}
    c.update(gamma=float(fl[0]), tau=float(fl[1]), auto=bool(fl[2]), log_ent_coef=float(fl[3]), ent_coef=float(fl[4]), target_entropy=float(fl[5]),
             hi=bool(fl[6]), arch=SC.ARCHS["golden"])
    out = {k[len(f"{name}/out/"):]: z[k] for k in z.files if k.startswith(f"{name}/out/")}
    return c, out


@lru_cache(maxsize=None)
def golden_reference(name):
    return SC.step_ref(golden_case(name)[0])


def all_cases():
    """Every case the GPU tests run: name -> (case, float64 reference)."""
    for name in SC.GPU_CASES:
        yield name, SC.gpu_case(name), SC.gpu_reference(name)
    for name in GOLDEN_CASES:
        yield "golden_" + name, golden_case(name)[0], golden_reference(name)


def test_symbols_are_declared_bound_and_versioned():
    hdr = open(os.path.join(ROOT, "include", "m3l_amd.h")).read()
    for s in SYMBOLS:
        assert s + "(" in hdr and s in L.EXPORTS and hasattr(L.lib(), s), s
    assert "typedef struct m3l_sac_desc" in hdr and "M3L_SAC_MAX_HIDDEN 3" in hdr and "SAC policy head (ABI 410)" in hdr
    lib = L.lib()
    assert lib.m3l_version() >= 410
    d = L.SacDesc()
    d.features, d.actions, d.n_pi, d.n_qf = 256, 7, 2, 2
    for l in range(2):
        d.pi_width[l] = d.qf_width[l] = 256
    # at least: 2 + 4 hidden activations and their gradients, the critics' input, and u, log_std and their gradients
    assert lib.m3l_sac_ws_bytes(C.byref(d), 256) >= 4 * (12 * 256 * 256 + 256 * 263 + 4 * 256 * 7)
    d.features = 40
    assert lib.m3l_sac_ws_bytes(C.byref(d), 256) == 256          # an unsupported shape sizes nothing
    d.features, d.actions = 256, 65
    assert lib.m3l_sac_ws_bytes(C.byref(d), 256) == 256


def test_descriptor_packing():
    """Field order and sizes of the ctypes mirror against the header's struct, and the pointers of a head in their slots."""
    assert [n for n, _ in L.SacDesc._fields_] == ["features", "actions", "n_pi", "n_qf", "pi_width", "qf_width", "pi_weight", "pi_bias", "mu_weight",
                                                  "mu_bias", "log_std_weight", "log_std_bias", "qf_weight", "qf_bias", "q_weight", "q_bias"]
    assert C.sizeof(L.SacDesc) == 10 * 4 + (3 + 3 + 4 + 6 + 6 + 2 + 2) * 8 and L.SacDesc.pi_weight.offset == 40
    arch = SC.ARCHS["mixed"]
    head = m3l_amd.SACHead(arch[0], arch[3], net_arch=dict(pi=list(arch[1]), qf=list(arch[2])))
    p = head.params()
    named = dict(head.named_parameters())
    assert [t.data_ptr() for t in p.actor_flat()] == [named[n].data_ptr() for n in SC.actor_names(arch)]
    assert [t.data_ptr() for t in p.critic_flat()] == [named[n].data_ptr() for n in SC.critic_names(arch)]
    assert [t.data_ptr() for t in p.critic_flat(True)] == [named[n].data_ptr() for n in SC.critic_names(arch, "critic_target")]
    a = SH._arch(arch[0], p)
    assert a == (32, 1, (32,), (64, 48, 16))
    d = SH._desc(a, actor=p.actor_flat(), critic=p.critic_flat(True))
    assert (d.features, d.actions, d.n_pi, d.n_qf, list(d.pi_width), list(d.qf_width)) == (32, 1, 1, 3, [32, 0, 0], [64, 48, 16])
    assert d.pi_weight[0] == head.actor.latent_pi[0].weight.data_ptr() and d.pi_bias[0] == head.actor.latent_pi[0].bias.data_ptr()
    assert d.mu_weight == head.actor.mu.weight.data_ptr() and d.log_std_bias == head.actor.log_std.bias.data_ptr()
    for c, net in enumerate((head.critic_target.qf0, head.critic_target.qf1)):
        assert [d.qf_weight[c][l] for l in range(3)] == [net[2 * l].weight.data_ptr() for l in range(3)]
        assert [d.qf_bias[c][l] for l in range(3)] == [net[2 * l].bias.data_ptr() for l in range(3)]
        assert d.q_weight[c] == net[6].weight.data_ptr() and d.q_bias[c] == net[6].bias.data_ptr()
    only_actor = SH._desc(a, actor=p.actor_flat())
    assert only_actor.q_weight[0] is None and only_actor.mu_weight is not None


def _sb3_like(features_dim, action_dim, pi, qf):
    """A hand-built policy with SB3's names behind the extractor, in the creation order of SB3 2.x's SACPolicy._build (actor, critic, critic_target;
    in the Actor latent_pi, mu, log_std)."""
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
        c.qf0, _ = seq(features_dim + action_dim, qf, 1)
        c.qf1, _ = seq(features_dim + action_dim, qf, 1)
        setattr(m, name, c)
    return m


@pytest.mark.parametrize("arch", ["a64", "a256", "mixed", "nohid", "aligned", "amax"])
def test_head_has_sb3_names_layouts_and_loads_strictly(arch):
    Fd, pi, qf, A = SC.ARCHS[arch]
    head = m3l_amd.SACHead(Fd, A, net_arch=dict(pi=list(pi), qf=list(qf)))
    ref = _sb3_like(Fd, A, pi, qf)
    sd, rd = head.state_dict(), ref.state_dict()
    assert list(sd.keys()) == list(rd.keys()) == SC.param_names(SC.ARCHS[arch])
    assert [tuple(v.shape) for v in sd.values()] == [tuple(v.shape) for v in rd.values()]
    assert tuple(sd["critic.qf0.0.weight"].shape)[1] == Fd + A
    assert all(isinstance(m, nn.ReLU) for i, m in enumerate(head.actor.latent_pi) if i % 2)
    assert all(isinstance(m, nn.ReLU) for i, m in enumerate(head.critic.qf1) if i % 2)
    # the target starts as a copy of the critic and takes no gradient
    for k in SC.critic_names(SC.ARCHS[arch]):
        assert torch.equal(sd[k], sd["critic_target." + k[len("critic."):]])
    assert [n for n, p in head.named_parameters() if p.requires_grad] == SC.actor_names(SC.ARCHS[arch]) + SC.critic_names(SC.ARCHS[arch])
    head.load_state_dict(rd, strict=True)
    assert "SACHead" in m3l_amd.__all__
    p = SH.SACHeadParams.from_policy(ref)          # an SB3-like object is read the same way
    assert [tuple(t.shape) for t in p.actor_flat() + p.critic_flat() + p.critic_flat(True)] == [tuple(v.shape) for v in rd.values()]


def test_default_architecture_and_init():
    torch.manual_seed(0)
    head = m3l_amd.SACHead(256, 7)
    assert [tuple(p.shape) for p in head.actor.parameters()] == [(256, 256), (256,), (256, 256), (256,), (7, 256), (7,), (7, 256), (7,)]
    assert [tuple(p.shape) for p in head.critic.qf0.parameters()] == [(256, 263), (256,), (256, 256), (256,), (1, 256), (1,)]
    # torch's nn.Linear default: uniform within 1 / sqrt(fan_in)
    w = head.critic.qf0[0].weight.detach()
    assert float(w.abs().max()) <= 263 ** -0.5 and float(w.abs().max()) > 0.9 * 263 ** -0.5


def test_cpu_tensors_raise_and_nothing_falls_back():
    head = m3l_amd.SACHead(64, 3, net_arch=dict(pi=[64], qf=[64]))
    x, a, v = torch.zeros(4, 64), torch.zeros(4, 3), torch.zeros(4)
    for call in (lambda: head(x), lambda: head.action_log_prob(x), lambda: head.q_values(x, a), lambda: head.td_target(x, v, v, 0.99, ent_coef=0.1),
                 lambda: head.critic_loss(x, a, v), lambda: head.actor_loss(x, ent_coef=0.1), lambda: head.ent_coef_loss(torch.zeros(1), v, -3.0),
                 lambda: head.polyak_update(0.005), lambda: SH.critic_loss_from(torch.zeros(2, 4), v), lambda: SH.actor_loss_from(v, torch.zeros(2, 4), 0.1)):
        with pytest.raises(m3l_amd.M3LError):
            call()


def test_every_refusal_carries_its_reason():
    H = m3l_amd.SACHead
    for kw, why in ((dict(features_dim=40), "multiples of 16"), (dict(features_dim=528), "at most 512"),
                    (dict(net_arch=dict(pi=[24], qf=[64])), "multiples of 16"), (dict(net_arch=dict(pi=[64], qf=[1024])), "at most 512"),
                    (dict(action_dim=0), "1 to 64"), (dict(action_dim=65), "1 to 64"), (dict(action_dim=2.5), "integer"),
                    (dict(net_arch=dict(pi=[16] * 4, qf=[16])), "0 to 3 hidden layers"), (dict(net_arch=dict(pi=[16], qf=[16] * 4)), "0 to 3 hidden layers"),
                    (dict(n_critics=3), "exactly 2 critics"), (dict(n_critics=1), "exactly 2 critics"), (dict(activation_fn=nn.Tanh), "ReLU only"),
                    (dict(use_sde=True), "use_sde"), (dict(share_features_extractor=False), "share_features_extractor=False")):
        args = dict(features_dim=64, action_dim=3)
        args.update(kw)
        with pytest.raises(ValueError, match=why):
            H(**args)
    # an SB3-like object outside the limits
    m = _sb3_like(64, 3, (64,), (64,))
    m.actor.latent_pi[1] = nn.Tanh()
    with pytest.raises(ValueError, match="ReLU only"):
        SH.SACHeadParams.from_policy(m)
    m = _sb3_like(64, 3, (64,), (64,))
    m.critic.qf2 = m.critic.qf1
    with pytest.raises(ValueError, match="exactly 2 critics"):
        SH.SACHeadParams.from_policy(m)
    m = _sb3_like(64, 3, (64,), (64,))
    m.actor.use_sde = True
    with pytest.raises(ValueError, match="use_sde"):
        SH.SACHeadParams.from_policy(m)
    m = _sb3_like(64, 3, (64,), (64,))
    m.actor.log_std = nn.Parameter(torch.zeros(3))
    with pytest.raises(ValueError, match="state-dependent log_std"):
        SH.SACHeadParams.from_policy(m)
    m = _sb3_like(64, 3, (64,), (64,))
    m.critic.share_features_extractor = False
    with pytest.raises(ValueError, match="share_features_extractor=False"):
        SH.SACHeadParams.from_policy(m)
    m = _sb3_like(64, 3, (64,), (64,)).double()
    with pytest.raises(ValueError, match="float32"):
        SH._arch(64, SH.SACHeadParams.from_policy(m))
    m = _sb3_like(64, 3, (64,), (64,))
    m.critic_target.qf1, _ = _sb3_like(64, 3, (64,), (32,)).critic.qf1, None
    with pytest.raises(ValueError, match="must be alike"):
        SH._arch(64, SH.SACHeadParams.from_policy(m))
    m = _sb3_like(64, 3, (64,), (64,))
    with pytest.raises(ValueError, match="do not follow an input of width"):
        SH._arch(48, SH.SACHeadParams.from_policy(m))
    with pytest.raises(ValueError, match="one of the two"):
        SH._ent_args(None, None)
    with pytest.raises(ValueError, match="one of the two"):
        SH._ent_args(0.1, torch.zeros(1))


@pytest.mark.parametrize("name", GOLDEN_CASES)
def test_restatement_equals_the_recorded_train_step(name):
    """tests/sac_cases.step_ref against what the reference's own SAC_MAE.train computed, to 1e-12 (relative to each tensor's largest entry)."""
    c, rec = golden_case(name)
    ref = golden_reference(name)

    def close(what, got, want):
        got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
        scale = max(1.0, float(np.abs(want).max()))
        assert got.shape == want.shape and float(np.abs(got - want).max()) <= 1e-12 * scale, (name, what, float(np.abs(got - want).max()))
    for k in ("a_pi", "log_prob", "target_q", "actor_loss", "critic_loss"):
        close(k, ref[k], rec[k])
    close("ent_coef", ref["ent_coef"], rec["ent_coef"])
    if c["auto"]:
        close("ent_coef_loss", ref["ent_coef_loss"], rec["ent_coef_loss"])
    else:
        assert "ent_coef_loss" not in rec and "grad/log_ent_coef" not in rec
    recorded = {k[len("grad/"):] for k in rec if k.startswith("grad/")}
    assert recorded == set(ref["grad"]) and recorded >= set(SC.actor_names(c["arch"]) + SC.critic_names(c["arch"]) + ["x"])
    for k in recorded:
        close("grad " + k, ref["grad"][k], rec["grad/" + k])
    assert {k[len("target/"):] for k in rec if k.startswith("target/")} == set(ref["target"])
    for k, v in ref["target"].items():
        close("target " + k, v, rec["target/" + k])


def test_restatement_equals_normal_and_the_closed_forms():
    c = SC.gpu_case("a64_b33")
    P = SC.as_torch(c["params"])
    x, noise = torch.from_numpy(c["x"]).double(), torch.from_numpy(c["noise_pi"]).double()
    with torch.no_grad():
        o = SC.actor_forward(P, x, noise)
        st = SC.actor_forward(P, x, noise, stable=True)
        s = torch.clamp(o["s_pre"], SC.LOG_STD_MIN, SC.LOG_STD_MAX)
        dist = torch.distributions.Normal(o["mu"], s.exp())
        lp = dist.log_prob(o["u"]).sum(1) - torch.log(1 - torch.tanh(o["u"]) ** 2 + 1e-6).sum(1)
        assert torch.allclose(o["log_prob"], lp, rtol=0, atol=1e-12)
        assert torch.allclose(o["log_prob"], SC.closed_form_log_prob(o["mu"], s, o["u"]), rtol=0, atol=1e-11)
        assert torch.allclose(o["log_prob"], st["log_prob"], rtol=0, atol=1e-9)          # the kernels' form is the same function
        assert torch.equal(o["actions"], torch.tanh(o["mu"] + s.exp() * noise))
        det = SC.actor_forward(P, x, torch.zeros_like(noise))
        assert torch.equal(det["actions"], torch.tanh(o["mu"]))
    # the stable 1 - tanh^2 and its derivative in u, as the header states them
    u = torch.linspace(-6, 6, 241, dtype=torch.float64, requires_grad=True)
    om = SC.stable_one_minus_tanh2(u)
    assert torch.allclose(om, 1 - torch.tanh(u) ** 2, rtol=1e-12, atol=1e-15)
    (-torch.log(1 - torch.tanh(u) ** 2 + 1e-6)).sum().backward()
    want = 2 * torch.tanh(u) * om / (om + 1e-6)
    assert torch.allclose(u.grad, want.detach(), rtol=1e-9, atol=1e-12)
    # clamp: gradient 1 on the closed interval, 0 outside
    v = torch.tensor([-20.0, 2.0, 2.0 + 1e-9, -20.0 - 1e-9, 0.0], dtype=torch.float64, requires_grad=True)
    torch.clamp(v, SC.LOG_STD_MIN, SC.LOG_STD_MAX).sum().backward()
    assert v.grad.tolist() == [1.0, 1.0, 0.0, 0.0, 1.0]


def test_input_conditions_of_every_gpu_case():
    """What the GPU comparisons rest on, for every case they use: gate, tie and clamp margins in float64; the float32 restatement (in the kernels'
    stable form) has the same gates and stays within a quarter of each bound; the measured pre-activation error is at most an eighth of the margin;
    the cases are trained-like."""
    assert SC.GATE_MARGIN >= 8 * SC.MEASURED_PRE_ERR
    worst_pre, hi_seen = 0.0, set()
    for name, c, ref in all_cases():
        cond = SC.conditions(ref)
        assert cond["gate"] >= SC.GATE_MARGIN and cond["tie"] >= SC.TIE_MARGIN and cond["clamp"] >= SC.CLAMP_MARGIN, (name, cond)
        if ref["pre"]:
            assert 0.1 <= cond["saturated"] <= 0.35, (name, cond)
        if c["hi"]:
            assert cond["above_clamp"] >= 0.05, (name, cond)
            hi_seen.add(name.split("_")[0])
        B = c["x"].shape[0]
        if B > 1:
            assert set(c["dones"].tolist()) == {0.0, 1.0}, name
        f32 = SC.step_ref(c, torch.float32, stable=True)
        for a, b in zip(f32["pre"], ref["pre"]):
            assert np.array_equal(a > 0, b > 0), (name, "a float32 gate differs from the float64 gate")
            worst_pre = max(worst_pre, float(np.abs(a - b).max()))
        for a, b in zip(f32["s_pre"], ref["s_pre"]):
            assert np.array_equal((a >= -20) & (a <= 2), (b >= -20) & (b <= 2)), name
        assert np.array_equal(f32["q_pi"][0] <= f32["q_pi"][1], ref["q_pi"][0] <= ref["q_pi"][1]), name
        assert np.array_equal(f32["q_next"][0] <= f32["q_next"][1], ref["q_next"][0] <= ref["q_next"][1]), name
        for k in ("a_pi", "log_prob", "ent_coef", "target_q", "q_replay", "q_pi", "critic_loss", "actor_loss") + (("ent_coef_loss",) if c["auto"] else ()):
            err = float((np.abs(f32[k] - ref[k]) / np.maximum(1.0, np.abs(ref[k]))).max())
            assert err <= VALUE_TOL / 4, (name, k, err)
        for k, r in ref["grad"].items():
            gmax = float(np.abs(r).max())
            assert gmax > 0 and float(np.abs(f32["grad"][k] - r).max()) <= GRAD_TOL / 4 * gmax, (name, k)
    assert hi_seen >= {"a64", "a256", "mixed", "nohid", "aligned", "amax", "golden"}
    assert worst_pre <= SC.MEASURED_PRE_ERR, worst_pre
    assert max(np.abs(u).max() for n in SC.GPU_CASES for u in SC.gpu_reference(n)["u"] if not SC.gpu_case(n)["hi"]) >= 3.0


def test_case_table_covers_what_the_issue_lists():
    b = lambda arch: sorted(B for a, B, _, _ in SC.GPU_CASES.values() if a == arch)      # noqa: E731
    assert b("a64") == [1, 2, 3, 15, 17, 33, 63, 65] and b("a256") == [130]
    for arch in ("mixed", "nohid", "aligned", "amax"):
        assert 2 <= len(b(arch)) <= 3 and set(b(arch)) <= {1, 3, 15, 33, 65}
    assert sorted((SC.ARCHS[a][0] + SC.ARCHS[a][3]) % 4 for a in ("a64", "mixed", "nohid", "aligned")) == [0, 1, 2, 3]
    assert {auto for _, _, _, auto in SC.GPU_CASES.values()} == {True, False}
