"""GPU checks of the PPO policy head (m3l_policy_*, m3l_amd.ActorCriticHead, m3l_amd/policy.py).

Yardsticks: the float64 restatement of tests/ppo_cases.py, which test_policy_head_cpu.py pins to the results recorded from the reference's own
`PPO_MAE.train` (tests/golden/ppo_head_step.npz) to 1e-12, and those records themselves.  Every input satisfies the conditions that
test_policy_head_cpu.py asserts for it: no ratio within 1e-3 of 1 +- clip_range and no |v - v_old| within 1e-3 of clip_range_vf, so the clipped
rows are the same rows in float32 and float64 and clip_fraction is compared exactly; the reference's own float32 run stays within a quarter of
each bound.  Bounds, the project's float32 bars (test_koleo_gpu.py, test_sinkhorn_gpu.py): loss, statistics, values / log_prob / entropy
1e-4 max(1, |ref|); every gradient tensor (dx and d log_std included) 1e-4 of its largest float64 entry."""
import ctypes as C

import numpy as np
import pytest
import torch

import m3l_amd
import memguard as MG
import ppo_cases as PC
from m3l_amd import _lib as L
from m3l_amd import policy as PH
from test_policy_head_cpu import GOLDEN_CASES, _sb3_like, golden_case

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
VALUE_TOL = GRAD_TOL = 1e-4
ALL = list(PC.GPU_CASES)


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _head(c):
    Fd, pi, vf, A = c["arch"]
    head = m3l_amd.ActorCriticHead(Fd, A, net_arch=dict(pi=list(pi), vf=list(vf)))
    head.load_state_dict({k: torch.from_numpy(v) for k, v in c["params"].items()}, strict=True)
    return head.to(DEV)


def _t(c, k):
    return torch.from_numpy(c[k]).to(DEV)


def _loss_kw(c):
    return dict(clip_range=c["clip_range"], ent_coef=c["ent_coef"], vf_coef=c["vf_coef"], clip_range_vf=c["clip_range_vf"],
                old_values=_t(c, "old_values") if c["clip_range_vf"] is not None else None, normalize_advantage=c["normalize_advantage"])


def _check_values(what, got, ref):
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    err = float((np.abs(got - ref) / np.maximum(1.0, np.abs(ref))).max())
    print(f"[{what}] err {err:.2e} (bound {VALUE_TOL:.0e})")
    assert got.shape == ref.shape and err <= VALUE_TOL, (what, err)


def _check_grads(what, got, ref):
    """got: {name: tensor}, ref: {name: float64 array}; every tensor within GRAD_TOL of its largest float64 entry."""
    assert set(got) == set(ref), set(got) ^ set(ref)
    worst = ("", 0.0)
    for k, r in ref.items():
        g = got[k].detach().double().cpu().numpy()
        gmax = float(np.abs(r).max())
        err = float(np.abs(g - r).max()) / gmax if gmax > 0 else (0.0 if not np.any(g) else float("inf"))
        if err >= worst[1]:
            worst = (k, err)
        assert g.shape == r.shape and err <= GRAD_TOL, (what, k, err, gmax)
    print(f"[{what}] gradient err worst {worst[1]:.2e} of the largest entry at {worst[0]} (bound {GRAD_TOL:.0e})")


def _loss_run(c, head=None, dloss=None):
    """ppo_loss forward + backward on a case -> (loss, stats tensor, {name: grad}) on the CPU."""
    head = head or _head(c)
    for p in head.parameters():
        p.grad = None
    x = _t(c, "x").requires_grad_(True)
    loss, stats = head.ppo_loss(x, _t(c, "actions"), _t(c, "old_log_prob"), _t(c, "advantages"), _t(c, "returns"), **_loss_kw(c))
    (loss if dloss is None else loss * dloss).backward()
    torch.cuda.synchronize()
    grads = {n: p.grad.cpu() for n, p in head.named_parameters()}
    grads["x"] = x.grad.cpu()
    return loss.detach().cpu(), stats, grads


def _check_loss(what, c, ref_loss, ref_stats, ref_count, ref_grads, run):
    loss, stats, grads = run
    assert loss.dtype == torch.float32 and loss.dim() == 0 and stats.shape == (5,) and stats.is_cuda and not stats.requires_grad
    sd = stats.stats_dict()
    assert list(sd) == list(PC.STAT_NAMES) and all(isinstance(v, float) for v in sd.values())
    _check_values(what + " loss", float(loss), ref_loss)
    for k in PC.STAT_NAMES:
        if k != "clip_fraction":
            _check_values(f"{what} {k}", sd[k], ref_stats[k])
    B = c["x"].shape[0]
    assert sd["clip_fraction"] == float(np.float32(ref_count) / np.float32(B)), (sd["clip_fraction"], ref_count, B)
    _check_grads(what, grads, ref_grads)


@pytest.mark.parametrize("name", ALL)
def test_evaluate_actions_forward_and_backward_against_the_restatement(name):
    """Measured on an MI355X (EXPERIMENTS.md 5.17): values / log_prob / entropy within 2.5e-6 (bound 1e-4), gradients within 5.7e-6 of the largest
    entry (bound 1e-4); two runs equal in every bit."""
    c = PC.gpu_case(name)
    B = c["x"].shape[0]
    g = torch.Generator().manual_seed(7)
    dv, dl, de = (torch.randn(B, generator=g) for _ in range(3))
    ref = PC.eval_ref(c, dv.numpy(), dl.numpy(), de.numpy())
    head = _head(c)
    runs = []
    for _ in range(2):
        for p in head.parameters():
            p.grad = None
        x = _t(c, "x").requires_grad_(True)
        values, logp, ent = head.evaluate_actions(x, _t(c, "actions"))
        assert values.shape == logp.shape == ent.shape == (B,) and values.dtype == torch.float32
        torch.autograd.backward([values, logp, ent], [dv.to(DEV), dl.to(DEV), de.to(DEV)])
        torch.cuda.synchronize()
        grads = {n: p.grad.cpu() for n, p in head.named_parameters()}
        grads["x"] = x.grad.cpu()
        runs.append(((values.detach().cpu(), logp.detach().cpu(), ent.detach().cpu()), grads))
    assert all(torch.equal(a, b) for a, b in zip(runs[0][0], runs[1][0])), "two runs differ in their bits (outputs)"
    assert all(torch.equal(runs[0][1][k], runs[1][1][k]) for k in runs[0][1]), "two runs differ in their bits (gradients)"
    for k, got in zip(("values", "log_prob", "entropy"), runs[0][0]):
        _check_values(f"{name} {k}", got.numpy(), ref[k])
    _check_grads(name, runs[0][1], ref["grad"])
    with torch.no_grad():                       # no workspace, no stores: the same bits
        again = head.evaluate_actions(_t(c, "x"), _t(c, "actions"))
    assert all(torch.equal(a.cpu(), b) for a, b in zip(again, runs[0][0]))
    assert torch.equal(head.predict_values(_t(c, "x")).cpu(), runs[0][0][0])


@pytest.mark.parametrize("name", GOLDEN_CASES)
def test_evaluate_actions_against_the_recorded_train_step(name):
    c, out = golden_case(name)
    head = _head(c)
    values, logp, ent = head.evaluate_actions(_t(c, "x"), _t(c, "actions"))
    for k, got in (("values", values), ("log_prob", logp), ("entropy", ent)):
        _check_values(f"golden {name} {k}", got.detach().cpu().numpy(), out[k])


@pytest.mark.parametrize("name", ALL)
def test_ppo_loss_against_the_restatement(name):
    """Measured on an MI355X (EXPERIMENTS.md 5.17): loss and statistics within 1.2e-6 (bound 1e-4), gradients within 5.7e-6 of the largest entry
    (bound 1e-4), clip_fraction equal to count / B in every case."""
    c, ref = PC.gpu_case(name), PC.gpu_reference(name)
    head = _head(c)
    a, b = _loss_run(c, head), _loss_run(c, head)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1].cpu(), b[1].cpu()) and all(torch.equal(a[2][k], b[2][k]) for k in a[2]), "two runs differ in their bits"
    _check_loss(name, c, ref["loss"], ref, ref["clip_count"], ref["grad"], a)


@pytest.mark.parametrize("name", GOLDEN_CASES)
def test_ppo_loss_against_the_recorded_train_step(name):
    """The four flag combinations as the reference's own PPO_MAE.train computed them in float64."""
    c, out = golden_case(name)
    B = c["x"].shape[0]
    count = int(round(float(out["clip_fraction"]) * B))
    grads = {k[len("grad/"):]: out[k] for k in out if k.startswith("grad/")}
    _check_loss("golden " + name, c, float(out["loss"]), {k: float(out[k]) for k in PC.STAT_NAMES}, count, grads, _loss_run(c))


@pytest.mark.parametrize("name", ["a64_b17", "a64_b33", "a256_b130", "mixed_b65", "nopi_b63", "a64_b1"])
def test_eval_node_followed_by_the_loss_in_torch_agrees_with_the_fused_loss(name):
    c, ref = PC.gpu_case(name), PC.gpu_reference(name)
    head = _head(c)
    x = _t(c, "x").requires_grad_(True)
    values, logp, ent = head.evaluate_actions(x, _t(c, "actions"))
    kw = _loss_kw(c)
    r = PC.ppo_loss_ref(values, logp, ent, _t(c, "old_log_prob"), _t(c, "advantages"), _t(c, "returns"), c["clip_range"], c["ent_coef"], c["vf_coef"],
                        c["clip_range_vf"], kw["old_values"], c["normalize_advantage"])
    r["loss"].backward()
    torch.cuda.synchronize()
    grads = {n: p.grad.cpu() for n, p in head.named_parameters()}
    grads["x"] = x.grad.cpu()
    _check_values(name + " torch loss", float(r["loss"].detach()), ref["loss"])
    assert int(r["clip_count"]) == ref["clip_count"]
    _check_grads(name + " torch loss", grads, ref["grad"])
    fused = _loss_run(c, head)
    _check_values(name + " fused vs torch loss", float(fused[0]), float(r["loss"].detach()))
    for k in grads:
        gmax = float(np.abs(ref["grad"][k]).max())
        assert float((fused[2][k] - grads[k]).abs().max()) <= GRAD_TOL * gmax, k


@pytest.mark.parametrize("name", ["a64_b17", "a256_b130", "mixed_b33", "nopi_b3"])
def test_first_epoch_identity(name):
    """old_log_prob taken from evaluate_actions on the same inputs: every ratio is exactly 1."""
    c = dict(PC.gpu_case(name))
    head = _head(c)
    with torch.no_grad():
        _, logp, _ = head.evaluate_actions(_t(c, "x"), _t(c, "actions"))
    c["old_log_prob"] = logp.cpu().numpy()
    loss, stats, grads = _loss_run(c, head)
    sd = stats.stats_dict()
    assert sd["clip_fraction"] == 0.0 and sd["approx_kl"] == 0.0
    wide = dict(c, clip_range=1e9)                 # nothing can be clipped: the unclipped gradient
    loss_w, _, grads_w = _loss_run(wide, head)
    assert torch.equal(loss, loss_w) and all(torch.equal(grads[k], grads_w[k]) for k in grads)
    c64 = dict(c, old_log_prob=c["old_log_prob"])
    P = PC.as_torch(c["params"])
    with torch.no_grad():
        lp64 = PC.head_forward(P, torch.from_numpy(c["x"]).double(), torch.from_numpy(c["actions"]).double())["log_prob"]
    # float64 yardstick with ITS ratio exactly 1: old_log_prob is handed over in float64
    Pg = PC.as_torch(c["params"], requires_grad=True)
    x = torch.from_numpy(c["x"]).double().requires_grad_(True)
    h = PC.head_forward(Pg, x, torch.from_numpy(c["actions"]).double())
    t = lambda k: torch.from_numpy(c64[k]).double()      # noqa: E731
    r = PC.ppo_loss_ref(h["values"], h["log_prob"], h["entropy"], lp64, t("advantages"), t("returns"), c["clip_range"], c["ent_coef"], c["vf_coef"],
                        c["clip_range_vf"], t("old_values") if c["clip_range_vf"] is not None else None, c["normalize_advantage"])
    r["loss"].backward()
    assert int(r["clip_count"]) == 0 and float(r["approx_kl"]) == 0.0
    ref = {k: p.grad.numpy() for k, p in Pg.items()}
    ref["x"] = x.grad.numpy()
    _check_values(name + " first epoch loss", float(loss), float(r["loss"].detach()))
    _check_grads(name + " first epoch", grads, ref)


@pytest.mark.parametrize("name", ["a64_b3", "a64_b17", "a256_b130", "mixed_b65", "nopi_b63"])
def test_act(name):
    c, ref = PC.gpu_case(name), PC.gpu_reference(name)
    head = _head(c)
    B, A = c["actions"].shape
    x = _t(c, "x")
    noise = torch.randn(B, A, generator=torch.Generator().manual_seed(11))
    actions, values, logp = head(x, noise=noise.to(DEV))
    assert actions.shape == (B, A) and values.shape == (B,) and logp.shape == (B,) and not actions.requires_grad
    want = ref["mean"] + np.exp(c["params"]["log_std"].astype(np.float64)) * noise.double().numpy()
    _check_values(name + " actions", actions.cpu().numpy(), want)
    _check_values(name + " values", values.cpu().numpy(), ref["values"])
    for grad_mode in (False, True):
        with torch.set_grad_enabled(grad_mode):
            v2, lp2, _ = head.evaluate_actions(x, actions)
        assert torch.equal(lp2.detach(), logp), "log_prob of act differs from evaluate_actions on the returned actions"
        assert torch.equal(v2.detach(), values)
    mu, v3, lp3 = head(x, deterministic=True)
    _check_values(name + " deterministic", mu.cpu().numpy(), ref["mean"])
    mu0, _, lp0 = head(x, noise=torch.zeros(B, A, device=DEV))
    assert torch.equal(mu, mu0) and torch.equal(lp3, lp0) and torch.equal(v3, values)
    drawn = head(x)                                # the module draws its own noise
    assert drawn[0].shape == (B, A) and bool(torch.isfinite(drawn[2]).all())


def _abi_buffers(c, fill=None):
    """Descriptor, inputs and freshly allocated outputs of the C ABI for a case."""
    head = _head(c)
    flat = [PH._dev(t) for t in head.params().flat()]
    x, a = _t(c, "x"), _t(c, "actions")
    arch = PH._arch(x, head.params())
    B = x.shape[0]
    e = (lambda *s: torch.empty(*s, device=DEV)) if fill is None else (lambda *s: torch.full(s, fill, device=DEV))
    o = dict(values=e(B), logp=e(B), entropy=e(B), loss=e(1), stats=e(5), c_logp=e(B), c_v=e(B), dlogp=e(B), dvalues=e(B), dentropy=e(B), dx=e(*x.shape),
             actions=e(*a.shape))
    return head, flat, arch, x, a, B, o


def test_c_abi_dloss_scales_every_gradient_by_exactly_one_half():
    c = PC.gpu_case("a64_b33")
    head, flat, arch, x, a, B, o = _abi_buffers(c)
    lib = L.lib()
    d = PH._desc(arch, flat)
    ws = torch.empty(int(lib.m3l_policy_ws_bytes(C.byref(d), B)), dtype=torch.uint8, device=DEV)
    assert lib.m3l_policy_eval_fwd(C.byref(d), B, L.ptr(x), L.ptr(a), L.ptr(ws), L.ptr(o["values"]), L.ptr(o["logp"]), L.ptr(o["entropy"]), _stream()) == 0, \
        L.last_error()
    assert lib.m3l_policy_ppo_loss_fwd(L.ptr(o["logp"]), L.ptr(o["values"]), L.ptr(o["entropy"]), L.ptr(_t(c, "old_log_prob")), L.ptr(_t(c, "advantages")),
                                       L.ptr(_t(c, "returns")), None, B, c["clip_range"], -1.0, c["ent_coef"], c["vf_coef"], 0, L.ptr(o["loss"]),
                                       L.ptr(o["stats"]), L.ptr(o["c_logp"]), L.ptr(o["c_v"]), _stream()) == 0, L.last_error()
    results = []
    for dl in (1.0, 0.5):
        dloss = torch.tensor([dl], device=DEV)
        grads = [torch.empty_like(t) for t in flat]
        gd = PH._desc(arch, grads)
        dx = torch.empty_like(x)
        assert lib.m3l_policy_ppo_loss_bwd(L.ptr(dloss), L.ptr(o["c_logp"]), L.ptr(o["c_v"]), B, c["ent_coef"], L.ptr(o["dlogp"]), L.ptr(o["dvalues"]),
                                           L.ptr(o["dentropy"]), _stream()) == 0, L.last_error()
        assert lib.m3l_policy_eval_bwd(C.byref(d), B, L.ptr(x), L.ptr(a), L.ptr(o["dvalues"]), L.ptr(o["dlogp"]), L.ptr(o["dentropy"]), L.ptr(ws), L.ptr(dx),
                                       C.byref(gd), _stream()) == 0, L.last_error()
        torch.cuda.synchronize()
        results.append([dx.clone()] + [g.clone() for g in grads])
    ref = PC.gpu_reference("a64_b33")
    names = ["x"] + PC.param_names(c["arch"])
    _check_grads("C ABI a64_b33", dict(zip(names, results[0])), ref["grad"])
    for n, full, half in zip(names, *results):
        assert float(full.abs().max()) > 0 and torch.equal(half, 0.5 * full), n


@pytest.mark.parametrize("bad", ["F=40", "A=65", "4 hidden layers", "width 24", "B=0"])
def test_c_abi_refuses_bad_shapes_and_writes_nothing(bad):
    """Buffers of a supported shape filled with a known value, the calls with the refused descriptor: an error, every byte as it was."""
    c = PC.gpu_case("a64_b17")
    head, flat, arch, x, a, B, o = _abi_buffers(c, fill=7.0)
    lib = L.lib()
    good = PH._desc(arch, flat)
    nb = int(lib.m3l_policy_ws_bytes(C.byref(good), B))
    ws = torch.full((nb,), 0x5A, dtype=torch.uint8, device=DEV)
    grads = [torch.full_like(t, 7.0) for t in flat]
    d, gd = PH._desc(arch, flat), PH._desc(arch, grads)
    for desc in (d, gd):
        if bad == "F=40":
            desc.features = 40
        elif bad == "A=65":
            desc.actions = 65
        elif bad == "4 hidden layers":
            desc.n_pi = 4
        elif bad == "width 24":
            desc.vf_width[1] = 24
    Bc = 0 if bad == "B=0" else B
    assert lib.m3l_policy_ws_bytes(C.byref(d), Bc) == 256
    rcs = [lib.m3l_policy_eval_fwd(C.byref(d), Bc, L.ptr(x), L.ptr(a), L.ptr(ws), L.ptr(o["values"]), L.ptr(o["logp"]), L.ptr(o["entropy"]), _stream())]
    assert "unsupported shape" in L.last_error() and "policy_eval_fwd" in L.last_error()
    rcs.append(lib.m3l_policy_act(C.byref(d), Bc, L.ptr(x), None, L.ptr(o["actions"]), L.ptr(o["values"]), L.ptr(o["logp"]), _stream()))
    assert "unsupported shape" in L.last_error() and "policy_act" in L.last_error()
    rcs.append(lib.m3l_policy_eval_bwd(C.byref(d), Bc, L.ptr(x), L.ptr(a), L.ptr(o["dvalues"]), L.ptr(o["dlogp"]), L.ptr(o["dentropy"]), L.ptr(ws),
                                       L.ptr(o["dx"]), C.byref(gd), _stream()))
    assert "unsupported shape" in L.last_error() and "policy_eval_bwd" in L.last_error()
    if bad == "B=0":
        rcs.append(lib.m3l_policy_ppo_loss_fwd(L.ptr(o["logp"]), L.ptr(o["values"]), L.ptr(o["entropy"]), L.ptr(o["logp"]), L.ptr(o["logp"]), L.ptr(o["logp"]),
                                               None, 0, 0.2, -1.0, 0.0, 0.5, 1, L.ptr(o["loss"]), L.ptr(o["stats"]), L.ptr(o["c_logp"]), L.ptr(o["c_v"]),
                                               _stream()))
        rcs.append(lib.m3l_policy_ppo_loss_bwd(L.ptr(o["loss"]), L.ptr(o["c_logp"]), L.ptr(o["c_v"]), 0, 0.0, L.ptr(o["dlogp"]), L.ptr(o["dvalues"]),
                                               L.ptr(o["dentropy"]), _stream()))
    torch.cuda.synchronize()
    assert all(rc != 0 for rc in rcs), rcs
    assert all(bool((t == 7).all()) for t in list(o.values()) + grads) and bool((ws == 0x5A).all())


def test_python_refuses_heads_outside_the_limits_on_the_gpu():
    """The functions that take a foreign policy's parameters hold them to the kernels' limits before anything is launched."""
    c = PC.gpu_case("a64_b17")
    head = _head(c)
    narrow = PH.HeadParams.from_policy(_sb3_like(40, 3, (64,), (64,)).to(DEV))
    with pytest.raises(ValueError, match="multiples of 16"):
        PH.evaluate_actions(narrow, torch.zeros(4, 40, device=DEV), torch.zeros(4, 3, device=DEV))
    with pytest.raises(ValueError, match="multiples of 16"):
        PH.act(narrow, torch.zeros(4, 40, device=DEV))
    with pytest.raises(ValueError, match="hidden layers"):
        PH.act(PH.HeadParams.from_policy(_sb3_like(64, 3, (64,) * 4, (64,)).to(DEV)), torch.zeros(4, 64, device=DEV))
    with pytest.raises(ValueError, match="do not follow an input of width 48"):
        head.evaluate_actions(torch.zeros(4, 48, device=DEV), torch.zeros(4, 3, device=DEV))
    with pytest.raises(ValueError, match="actions"):
        head.evaluate_actions(_t(c, "x"), torch.zeros(17, 4, device=DEV))
    with pytest.raises(ValueError, match="clip_range_vf"):
        head.ppo_loss(_t(c, "x"), _t(c, "actions"), _t(c, "old_log_prob"), _t(c, "advantages"), _t(c, "returns"), 0.2, clip_range_vf=0.3)


@pytest.mark.parametrize("name", ["mixed_b33", "a64_b17"])
def test_memory_contract(monkeypatch, name):
    """Guarded, poisoned allocations at a ragged-tile shape: no write outside a buffer, no read of stale workspace or outputs."""
    c = PC.gpu_case(name)
    head = _head(c)
    x0 = _t(c, "x")
    noise = torch.randn(*c["actions"].shape, generator=torch.Generator().manual_seed(3)).to(DEV)

    def work(g):
        for p in head.parameters():
            p.grad = None
        x = x0.clone().requires_grad_(True)
        loss, stats = head.ppo_loss(x, _t(c, "actions"), _t(c, "old_log_prob"), _t(c, "advantages"), _t(c, "returns"), **_loss_kw(c))
        g.check("after the forward")
        loss.backward()
        g.check("after the backward")
        acted = head(x0, noise=noise)
        g.check("after act")
        return {"loss": loss, "stats": stats.as_subclass(torch.Tensor), "dx": x.grad, "grad": {n: p.grad for n, p in head.named_parameters()},
                "act": list(acted)}
    counts = MG.run_contract(monkeypatch, work)
    assert counts[0] == counts[1] and counts[0][0] == 1          # one workspace: the eval node's


@pytest.mark.parametrize("name", ["mixed_b33", "a256_b17"])
def test_evaluate_actions_under_no_grad_takes_no_workspace(monkeypatch, name):
    """Parameters that require a gradient, grad mode off: no workspace is sized or requested and no activation is stored; the outputs are the bits
    of the grad-mode call, whose forward requests exactly one workspace.  Guarded, poisoned allocations in both modes."""
    c = PC.gpu_case(name)
    head = _head(c)
    assert all(p.requires_grad for p in head.parameters())
    x, a = _t(c, "x"), _t(c, "actions")

    def no_grad(g):
        with torch.no_grad():
            out = head.evaluate_actions(x, a)
            values = head.predict_values(x)
        g.check("after evaluate_actions under no_grad")
        return {"out": list(out), "values": values}

    def grad(g):
        out = head.evaluate_actions(x, a)
        g.check("after evaluate_actions in grad mode")
        return {"out": [t.detach() for t in out]}
    sized = []
    lib = L.lib()
    real = lib.m3l_policy_ws_bytes
    monkeypatch.setattr(lib, "m3l_policy_ws_bytes", lambda *args: sized.append(1) or real(*args))
    counts = MG.run_contract(monkeypatch, no_grad, need_ws=False)
    assert all(n_ws == 0 for n_ws, _ in counts) and not sized, (counts, len(sized))
    counts = MG.run_contract(monkeypatch, grad)
    assert all(n_ws == 1 for n_ws, _ in counts) and len(sized) == 3          # the unguarded run and one per fill
    with torch.no_grad():
        quiet = head.evaluate_actions(x, a)
    loud = head.evaluate_actions(x, a)
    assert all(torch.equal(q, l.detach()) for q, l in zip(quiet, loud)) and not quiet[0].requires_grad and loud[0].requires_grad
    frozen = _head(c).requires_grad_(False)          # nothing requires a gradient: no workspace in grad mode either
    sized.clear()
    out = frozen.evaluate_actions(x, a)
    assert not sized and not out[0].requires_grad and all(torch.equal(q, o) for q, o in zip(quiet, out))
    sized.clear()
    out = frozen.evaluate_actions(x.clone().requires_grad_(True), a)          # the features alone do
    assert len(sized) == 1 and out[0].requires_grad


def test_end_to_end_extractor_head_loss():
    """MAEExtractor -> head -> ppo_loss(...).backward() against the same extractor with the restatement's head in float32 torch on the GPU: loss and
    head gradients within the bounds above, the encoder's parameter gradients within the extractor tests' float32 gradient bound
    (test_parity_gpu.py::test_mae_extractor_golden: 3e-3 of the largest entry + 1e-7)."""
    from m3l_amd import VTMAE, VTT, MAEExtractor
    D, fs, B, A = 64, 1, 5, 3
    torch.manual_seed(2)
    enc = VTT(image_size=32, tactile_size=16, image_patch_size=8, tactile_patch_size=4, dim=D, depth=1, heads=2, mlp_dim=128, image_channels=3 * fs,
              tactile_channels=3 * fs, num_tactiles=2, frame_stack=fs)
    mae = VTMAE(encoder=enc, decoder_dim=D, masking_ratio=0.75, decoder_depth=1, decoder_heads=2, num_tactiles=2, frame_stack=fs, compute_dtype="fp32")
    ext = MAEExtractor(mae, D, False, fs).to(DEV)
    g = torch.Generator().manual_seed(5)
    obs = {"image": torch.rand(B, fs, 32, 32, 3, generator=g).to(DEV), "tactile": (torch.rand(B, fs, 6, 16, 16, generator=g) * 2 - 1).to(DEV)}
    c = PC.make_inputs(PC.ARCHS["a64"], B, "vfclip", late=False, seed=77)
    head = _head(c)
    with torch.no_grad():
        feat0 = ext(obs)
        actions, values0, logp0 = head(feat0, noise=torch.randn(B, A, generator=g).to(DEV))
    # fixed offsets that keep every row well away from both clipping edges (ratios 0.95, 1.42, 0.74, 1.11, 0.67; |v - v_old| against 0.3)
    old_logp = logp0 + torch.tensor([0.05, -0.35, 0.3, -0.1, 0.4], device=DEV)
    old_values = values0 + torch.tensor([0.1, -0.45, 0.2, 0.5, -0.15], device=DEV)
    adv, ret = _t(c, "advantages"), values0 + _t(c, "returns") * 0.3
    kw = dict(clip_range=0.2, ent_coef=0.01, vf_coef=0.5, clip_range_vf=0.3, normalize_advantage=True)

    def grads_of():
        out = {"head." + n: p.grad.clone() for n, p in head.named_parameters()}
        out.update({"ext." + n: p.grad.clone() for n, p in ext.named_parameters() if p.grad is not None})
        for p in list(head.parameters()) + list(ext.parameters()):
            p.grad = None
        return out

    loss, stats = head.ppo_loss(ext(obs), actions, old_logp, adv, ret, old_values=old_values, **kw)
    loss.backward()
    got = grads_of()
    P = {n: p for n, p in head.named_parameters()}
    h = PC.head_forward(P, ext(obs), actions)
    r = PC.ppo_loss_ref(h["values"], h["log_prob"], h["entropy"], old_logp, adv, ret, kw["clip_range"], kw["ent_coef"], kw["vf_coef"], kw["clip_range_vf"],
                        old_values, True)
    r["loss"].backward()
    want = grads_of()
    torch.cuda.synchronize()
    ratio = r["ratio"].cpu().numpy()
    assert np.minimum(np.abs(ratio - 0.8), np.abs(ratio - 1.2)).min() > PC.MARGIN and \
        float(((h["values"].detach() - old_values).abs() - 0.3).abs().min()) > PC.MARGIN, "an input sits on a clipping edge"
    _check_values("end to end loss", float(loss.detach()), float(r["loss"].detach()))
    assert stats.stats_dict()["clip_fraction"] == float(np.float32(int(r["clip_count"])) / np.float32(B))
    assert set(got) == set(want) and any(k.startswith("ext.mae.") or k.startswith("ext.vit_layer.") for k in got)
    for k in want:
        gmax = float(want[k].abs().max())
        err = float((got[k] - want[k]).abs().max())
        bound = GRAD_TOL * gmax if k.startswith("head.") else 3e-3 * gmax + 1e-7
        assert err <= bound, (k, err, bound)
