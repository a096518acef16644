"""CPU-only checks of the PPO policy head: the C ABI declarations, the public surface (ActorCriticHead: SB3's names and layouts, every rejection),
the float64 restatement of tests/ppo_cases.py against the closed forms, against torch.distributions.Normal and against the results recorded from the
reference's own `PPO_MAE.train` (golden/ppo_head_step.npz, golden/make_golden_ppo_head.py), and, for every case the GPU tests use, the conditions
their comparisons rest on.  No kernel is launched here."""
import os
from functools import lru_cache

import numpy as np
import pytest
import torch
from torch import nn

import m3l_amd
import ppo_cases as PC
from m3l_amd import _lib as L
from m3l_amd import policy as PH

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ["m3l_policy_ws_bytes", "m3l_policy_act", "m3l_policy_eval_fwd", "m3l_policy_eval_bwd", "m3l_policy_ppo_loss_fwd", "m3l_policy_ppo_loss_bwd"]
GOLDEN_CASES = ["default", "vfclip", "nonorm", "b1"]
VALUE_TOL = GRAD_TOL = 1e-4        # the GPU tests' bounds (test_koleo_gpu.py, test_sinkhorn_gpu.py): 1e-4 max(1, |ref|); 1e-4 of a gradient's largest entry


@lru_cache(maxsize=None)
def _z():
    return np.load(os.path.join(ROOT, "tests", "golden", "ppo_head_step.npz"))


@lru_cache(maxsize=None)
def golden_case(name):
    """(case in the form of ppo_cases.make_inputs, recorded results) of a case of ppo_head_step.npz."""
    z = _z()
    flags = z[f"{name}/flags"]
    c = {k: z[f"{name}/in/{k}"] for k in ("x", "actions", "old_log_prob", "advantages", "returns", "old_values")}
    c["params"] = {k[len(f"{name}/param/"):]: z[k] for k in z.files if k.startswith(f"{name}/param/")}
    c.update(clip_range=float(flags[0]), clip_range_vf=None if flags[1] < 0 else float(flags[1]), normalize_advantage=bool(flags[2]),
             ent_coef=float(flags[3]), vf_coef=float(flags[4]), arch=PC.ARCHS["golden"], late=c["x"].shape[0] > 1)
    out = {k[len(f"{name}/out/"):]: z[k] for k in z.files if k.startswith(f"{name}/out/")}
    return c, out


def all_cases():
    """Every case the GPU tests run: name -> (case, float64 reference)."""
    for name in PC.GPU_CASES:
        yield name, PC.gpu_case(name), PC.gpu_reference(name)
    for name in GOLDEN_CASES:
        c, _ = golden_case(name)
        yield "golden_" + name, c, PC.run_ref(c)


def test_symbols_are_declared_bound_and_versioned():
    hdr = open(os.path.join(ROOT, "include", "m3l_amd.h")).read()
    for s in SYMBOLS:
        assert s + "(" in hdr and s in L.EXPORTS and hasattr(L.lib(), s), s
    assert "typedef struct m3l_policy_desc" in hdr and "M3L_POLICY_MAX_HIDDEN 3" in hdr
    lib = L.lib()
    assert lib.m3l_version() >= 409
    import ctypes as C
    d = L.PolicyDesc()
    d.features, d.actions, d.n_pi, d.n_vf = 256, 7, 2, 2
    for l in range(2):
        d.pi_width[l] = d.vf_width[l] = 256
    # at least: 4 hidden activations and their gradients, mu and d mu
    assert lib.m3l_policy_ws_bytes(C.byref(d), 512) >= 4 * (8 * 512 * 256 + 2 * 512 * 7)
    d.features = 40
    assert lib.m3l_policy_ws_bytes(C.byref(d), 512) == 256          # an unsupported shape sizes nothing


def _sb3_like(features_dim, action_dim, pi, vf):
    """A hand-built policy with SB3's names, in the creation order of SB3 2.x's ActorCriticPolicy._build."""
    def seq(widths):
        mods, k = [], features_dim
        for w in widths:
            mods += [nn.Linear(k, w), nn.Tanh()]
            k = w
        return nn.Sequential(*mods), k
    m = nn.Module()
    m.mlp_extractor = nn.Module()
    m.mlp_extractor.policy_net, kp = seq(pi)
    m.mlp_extractor.value_net, kv = seq(vf)
    m.action_net = nn.Linear(kp, action_dim)
    m.log_std = nn.Parameter(torch.zeros(action_dim))
    m.value_net = nn.Linear(kv, 1)
    return m


@pytest.mark.parametrize("arch", ["a64", "a256", "mixed", "nopi"])
def test_head_has_sb3_names_layouts_and_loads_strictly(arch):
    Fd, pi, vf, A = PC.ARCHS[arch]
    head = m3l_amd.ActorCriticHead(Fd, A, net_arch=dict(pi=list(pi), vf=list(vf)), log_std_init=-0.5)
    ref = _sb3_like(Fd, A, pi, vf)
    sd, rd = head.state_dict(), ref.state_dict()
    assert list(sd.keys()) == list(rd.keys())
    assert [tuple(v.shape) for v in sd.values()] == [tuple(v.shape) for v in rd.values()]
    assert [n for n, _ in head.named_parameters()] == [n for n, _ in ref.named_parameters()]
    assert set(sd.keys()) == set(PC.param_names(PC.ARCHS[arch]))
    assert all(isinstance(m, nn.Tanh) for i, m in enumerate(head.mlp_extractor.policy_net) if i % 2)
    assert all(isinstance(m, nn.Tanh) for i, m in enumerate(head.mlp_extractor.value_net) if i % 2)
    assert torch.equal(head.log_std.detach(), torch.full((A,), -0.5))
    head.load_state_dict(rd, strict=True)
    assert [t.data_ptr() for t in head.params().flat()] == [dict(head.named_parameters())[n].data_ptr() for n in PC.param_names(PC.ARCHS[arch])]
    assert "ActorCriticHead" in m3l_amd.__all__


def test_default_architecture_and_init():
    torch.manual_seed(0)
    head = m3l_amd.ActorCriticHead(64, 3)
    assert [tuple(p.shape) for p in head.mlp_extractor.policy_net.parameters()] == [(64, 64), (64,), (64, 64), (64,)]
    assert float(head.log_std.detach().abs().max()) == 0.0 and float(head.action_net.bias.detach().abs().max()) == 0.0
    w = head.mlp_extractor.policy_net[0].weight.detach().double()
    assert torch.allclose(w @ w.T, 2.0 * torch.eye(64, dtype=torch.float64), atol=1e-5)        # orthogonal, gain sqrt 2
    w = head.action_net.weight.detach().double()
    assert torch.allclose(w @ w.T, 1e-4 * torch.eye(3, dtype=torch.float64), atol=1e-9)


def test_cpu_tensors_raise_and_nothing_falls_back():
    head = m3l_amd.ActorCriticHead(64, 3)
    x, a = torch.zeros(4, 64), torch.zeros(4, 3)
    with pytest.raises(m3l_amd.M3LError):
        head(x)
    with pytest.raises(m3l_amd.M3LError):
        head.evaluate_actions(x, a)
    with pytest.raises(m3l_amd.M3LError):
        head.predict_values(x)
    with pytest.raises(m3l_amd.M3LError):
        head.ppo_loss(x, a, torch.zeros(4), torch.zeros(4), torch.zeros(4), 0.2)
    with pytest.raises(m3l_amd.M3LError):
        PH.ppo_loss_from(torch.zeros(4), torch.zeros(4), torch.zeros(4), torch.zeros(4), torch.zeros(4), torch.zeros(4), 0.2)


class _Discrete:
    n = 4


@pytest.mark.parametrize("kw,match", [
    (dict(activation_fn=nn.ReLU), "Tanh"),
    (dict(use_sde=True), "use_sde"),
    (dict(squash_output=True), "squash_output"),
    (dict(share_features_extractor=False), "share_features_extractor"),
    (dict(action_dim=_Discrete()), "discrete"),
    (dict(action_dim=3.0), "an integer expected"),
    (dict(action_dim=True), "an integer expected"),
    (dict(action_dim=65), "action_dim"),
    (dict(action_dim=0), "action_dim"),
    (dict(features_dim=40), "multiples of 16"),
    (dict(features_dim=528), "multiples of 16"),
    (dict(net_arch=dict(pi=[64, 40], vf=[64])), "multiples of 16"),
    (dict(net_arch=dict(pi=[64], vf=[1024])), "multiples of 16"),
    (dict(net_arch=dict(pi=[64] * 4, vf=[64])), "hidden layers"),
])
def test_rejections_carry_a_reason(kw, match):
    args = dict(features_dim=64, action_dim=3)
    args.update(kw)
    with pytest.raises(ValueError, match=match):
        m3l_amd.ActorCriticHead(**args)


def test_action_dim_may_be_any_integral_type():
    """`int(np.prod(space.shape))` left as a numpy integer is a continuous action vector's length, not a discrete space."""
    head = m3l_amd.ActorCriticHead(64, np.int64(3))
    assert head.action_dim == 3 and type(head.action_dim) is int and tuple(head.action_net.weight.shape) == (3, 64)


def test_parameters_of_another_dtype_are_refused_before_anything_runs():
    """A head kept in float64 or bf16 would get float32 gradients of copies: refused with the reason, forward and backward never start."""
    for dt in (torch.float64, torch.bfloat16):
        pol = _sb3_like(64, 3, (64,), (64,)).to(dt)
        with pytest.raises(ValueError, match="float32"):
            PH._arch(torch.zeros(2, 64), PH.HeadParams.from_policy(pol))
    pol = _sb3_like(64, 3, (64,), (64,))
    pol.log_std = nn.Parameter(torch.zeros(3, dtype=torch.float64))
    with pytest.raises(ValueError, match="float32"):
        PH._arch(torch.zeros(2, 64), PH.HeadParams.from_policy(pol))


def test_foreign_policies_are_checked_too():
    """The functions take an SB3-like policy's own parameters (HeadParams.from_policy): its configuration is held to the same rules."""
    pol = _sb3_like(64, 3, (64,), (64,))
    assert len(PH.HeadParams.from_policy(pol).flat()) == 9
    pol.mlp_extractor.policy_net[1] = nn.ReLU()
    with pytest.raises(ValueError, match="Tanh"):
        PH.HeadParams.from_policy(pol)
    for flag, value in (("use_sde", True), ("squash_output", True), ("share_features_extractor", False)):
        pol = _sb3_like(64, 3, (64,), (64,))
        setattr(pol, flag, value)
        with pytest.raises(ValueError, match=flag):
            PH.HeadParams.from_policy(pol)
    pol = _sb3_like(64, 3, (64,), (64,))
    del pol.log_std                                  # a categorical policy has none
    with pytest.raises(ValueError, match="continuous"):
        PH.HeadParams.from_policy(pol)
    pol = _sb3_like(40, 3, (64,), (64,))
    with pytest.raises(ValueError, match="multiples of 16"):
        PH._arch(torch.zeros(2, 40), PH.HeadParams.from_policy(pol))


@pytest.mark.parametrize("name", ["a64_b17", "a256_b17", "mixed_b33", "nopi_b63"])
def test_restatement_equals_the_closed_forms_and_the_normal_distribution(name):
    c = PC.gpu_case(name)
    P = PC.as_torch(c["params"])
    x, a = torch.from_numpy(c["x"]).double(), torch.from_numpy(c["actions"]).double()
    h = PC.head_forward(P, x, a)
    lp, en = PC.closed_forms(h["mean"], P["log_std"], a)
    dist = torch.distributions.Normal(h["mean"], P["log_std"].exp().expand_as(h["mean"]))
    for got, ref in ((h["log_prob"], lp), (h["entropy"], en), (h["log_prob"], dist.log_prob(a).sum(-1)), (h["entropy"], dist.entropy().sum(-1))):
        assert float((got - ref).abs().max()) <= 1e-12 * max(1.0, float(ref.abs().max()))
    # the gradient convention of the header, against autograd through min and clamp
    r = PC.gpu_reference(name)
    B = x.shape[0]
    lpt = torch.from_numpy(r["log_prob"]).requires_grad_(True)
    vt = torch.from_numpy(r["values"]).requires_grad_(True)
    t = lambda k: torch.from_numpy(c[k]).double()      # noqa: E731
    out = PC.ppo_loss_ref(vt, lpt, torch.from_numpy(r["entropy"]), t("old_log_prob"), t("advantages"), t("returns"), c["clip_range"], c["ent_coef"],
                          c["vf_coef"], c["clip_range_vf"], t("old_values") if c["clip_range_vf"] is not None else None, c["normalize_advantage"])
    out["loss"].backward()
    adv = t("advantages")
    if c["normalize_advantage"] and B > 1:
        adv = (adv - adv.mean()) / (adv.std() + 1e-8)
    ratio = torch.exp(lpt.detach() - t("old_log_prob"))
    open_ = adv * ratio <= adv * ratio.clamp(1 - c["clip_range"], 1 + c["clip_range"])
    assert float((lpt.grad - torch.where(open_, -adv * ratio / B, torch.zeros_like(adv))).abs().max()) <= 1e-12
    if c["clip_range_vf"] is None:
        dv = c["vf_coef"] * 2 * (vt.detach() - t("returns")) / B
    else:
        vp = t("old_values") + (vt.detach() - t("old_values")).clamp(-c["clip_range_vf"], c["clip_range_vf"])
        dv = torch.where((vt.detach() - t("old_values")).abs() <= c["clip_range_vf"], c["vf_coef"] * 2 * (vp - t("returns")) / B, torch.zeros_like(vp))
    assert float((vt.grad - dv).abs().max()) <= 1e-12
    # log_std: -ent_coef per dimension plus its share through log_prob
    share = (lpt.grad[:, None] * ((a - h["mean"]) ** 2 / torch.exp(2 * P["log_std"]) - 1)).sum(0)
    assert float((torch.from_numpy(r["grad"]["log_std"]) - (share - c["ent_coef"])).abs().max()) <= 1e-12


@pytest.mark.parametrize("name", GOLDEN_CASES)
def test_restatement_is_pinned_to_the_reference_train_step(name):
    """ppo_cases.run_ref on the recorded inputs against what the reference's own PPO_MAE.train computed in float64: outputs, logged losses and
    statistics, every parameter gradient and the gradient in the features, to 1e-12."""
    c, out = golden_case(name)
    r = PC.run_ref(c)
    B = c["x"].shape[0]
    assert c["x"].shape == ((24, 32) if name != "b1" else (1, 32)) and c["actions"].shape[1] == 3
    for k in ("values", "log_prob", "entropy"):
        assert float(np.abs(r[k] - out[k]).max()) <= 1e-12 * max(1.0, float(np.abs(out[k]).max())), k
    for k in ("loss", "policy_loss", "value_loss", "entropy_loss", "approx_kl"):
        assert abs(r[k] - float(out[k])) <= 1e-12 * max(1.0, abs(float(out[k]))), (k, r[k], float(out[k]))
    assert float(out["clip_fraction"]) == float(np.float32(r["clip_count"]) / np.float32(B))        # the reference averages a float32 mask (:298)
    names = [k[len("grad/"):] for k in out if k.startswith("grad/")]
    assert set(names) == set(PC.param_names(c["arch"])) | {"x"}
    for k in names:
        ref = out["grad/" + k]
        assert float(np.abs(r["grad"][k] - ref).max()) <= 1e-12 * max(1.0, float(np.abs(ref).max())), k


def test_recorded_flag_combinations_are_the_ones_asked_for():
    got = {n: (golden_case(n)[0]["clip_range_vf"], golden_case(n)[0]["normalize_advantage"], golden_case(n)[0]["x"].shape[0]) for n in GOLDEN_CASES}
    assert got == {"default": (None, True, 24), "vfclip": (PC.CLIP_RANGE_VF, True, 24), "nonorm": (None, False, 24), "b1": (None, True, 1)}
    assert os.path.getsize(os.path.join(ROOT, "tests", "golden", "ppo_head_step.npz")) < 512 * 1024


def test_case_grid_covers_the_tiling_edges():
    Bs = {PC.GPU_CASES[n][1] for n in PC.GPU_CASES}
    assert Bs == {1, 2, 3, 15, 17, 33, 63, 65, 130}
    assert {PC.GPU_CASES[n][0] for n in PC.GPU_CASES} == {"a64", "a256", "mixed", "nopi", "novf", "plain"}
    assert PC.ARCHS["a64"] == (64, (64, 64), (64, 64), 3) and PC.ARCHS["a256"] == (256, (256, 256), (256, 256), 7)
    assert PC.ARCHS["mixed"] == (32, (32,), (64, 48, 16), 1) and PC.ARCHS["nopi"] == (48, (), (16,), 2)
    assert PC.ARCHS["novf"] == (16, (16,), (), 1) and PC.ARCHS["plain"] == (16, (), (), 2)
    for arch in ("a64", "a256", "mixed", "nopi", "novf", "plain"):
        assert {PC.GPU_CASES[n][2] for n in PC.GPU_CASES if PC.GPU_CASES[n][0] == arch} >= {"default", "vfclip"}


@pytest.mark.parametrize("name,c,ref", [pytest.param(n, c, r, id=n) for n, c, r in all_cases()])
def test_conditions_the_gpu_comparisons_rest_on(name, c, ref):
    k = PC.conditions(c, ref)
    print(name, k)
    assert k["ratio_gap"] >= PC.MARGIN, "a ratio lies within 1e-3 of 1 +- clip_range"
    if c["clip_range_vf"] is not None:
        assert k["v_gap"] >= PC.MARGIN, "a |v - v_old| lies within 1e-3 of clip_range_vf"
    if c["late"]:
        assert 0.2 <= k["clipped_share"] <= 0.8, k["clipped_share"]
    if k["saturated"] is not None:
        assert k["saturated"] >= 0.10, "fewer than 10 % of the hidden units have |pre| > 2"
    assert k["action_sigmas"] <= 2.0 + 1e-6


@pytest.mark.parametrize("name,c,ref", [pytest.param(n, c, r, id=n) for n, c, r in all_cases()])
def test_float32_torch_stays_within_a_quarter_of_each_gpu_bound(name, c, ref):
    """The restatement in float32 torch (CPU) against its float64 run: the reference's own float32 error leaves three quarters of every bound
    to the kernels' summation order."""
    r32 = PC.run_ref(c, dtype=torch.float32)
    worst = {}
    for k in ("values", "log_prob", "entropy"):
        worst[k] = float((np.abs(r32[k] - ref[k]) / np.maximum(1.0, np.abs(ref[k]))).max())
    for k in ("loss",) + PC.STAT_NAMES:
        worst[k] = abs(r32[k] - ref[k]) / max(1.0, abs(ref[k]))
    for k, g in ref["grad"].items():
        gmax = float(np.abs(g).max())
        worst["grad/" + k] = float(np.abs(r32["grad"][k] - g).max()) / gmax if gmax > 0 else float(np.abs(r32["grad"][k]).max())
    print(name, {k: f"{v:.1e}" for k, v in worst.items()})
    assert r32["clip_count"] == ref["clip_count"]
    for k, v in worst.items():
        assert v <= 0.25 * (GRAD_TOL if k.startswith("grad/") else VALUE_TOL), (k, v)
