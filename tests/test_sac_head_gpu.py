"""GPU checks of the SAC policy head (m3l_sac_*, m3l_amd.SACHead, m3l_amd/sac.py).

Yardsticks: the float64 restatement of tests/sac_cases.py, which test_sac_head_cpu.py pins to the step recorded from the reference's own
`SAC_MAE.train` (tests/golden/sac_head_step.npz) to 1e-12, and those records themselves.  Every input satisfies the conditions that
test_sac_head_cpu.py asserts for it: every ReLU pre-activation at least GATE_MARGIN from 0, |q0 - q1| >= 1e-3 where a minimum is taken, no
pre-clamp log_std within 1e-3 of an edge, so the gates, the chosen critic and the clamp are the same in float32 and float64; the restatement's
own float32 run stays within a quarter of each bound.  Bounds, the project's float32 bars (test_policy_head_gpu.py): outputs, losses,
target_q and ent_coef 1e-4 max(1, |ref|); every gradient tensor 1e-4 of its largest float64 entry."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

import m3l_amd
import memguard as MG
import sac_cases as SC
from m3l_amd import _lib as L
from m3l_amd import sac as SH
from test_sac_head_cpu import GOLDEN_CASES, golden_case, golden_reference

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
VALUE_TOL = GRAD_TOL = 1e-4
ALL = list(SC.GPU_CASES)


def _head(c):
    Fd, pi, qf, A = c["arch"]
    head = m3l_amd.SACHead(Fd, A, net_arch=dict(pi=list(pi), qf=list(qf)))
    head.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in c["params"].items()}, strict=True)
    return head.to(DEV)


def _t(c, k):
    return torch.from_numpy(c[k]).to(DEV)


def _check_values(what, got, ref):
    got = got.detach().double().cpu().numpy() if isinstance(got, torch.Tensor) else np.asarray(got, dtype=np.float64)
    ref = np.asarray(ref, dtype=np.float64)
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


def _grads(head, prefix):
    return {n: p.grad for n, p in head.named_parameters() if n.startswith(prefix)}


def _clear(head):
    for p in head.parameters():
        p.grad = None


def _ent_kw(c, log_ent=None):
    if c["auto"]:
        return dict(log_ent_coef=log_ent if log_ent is not None else torch.tensor([c["log_ent_coef"]], dtype=torch.float32, device=DEV))
    return dict(ent_coef=c["ent_coef"])


@pytest.mark.parametrize("name", ALL)
def test_action_log_prob_forward_and_backward_against_the_restatement(name):
    """Random output gradients in the actions and the log-probability; two runs equal in every bit; the no_grad call gives the same bits; the
    deterministic action is tanh(mu).  Measured on an MI355X (EXPERIMENTS.md 5.18): actions / log_prob within 3.0e-6 (bound 1e-4), gradients
    within 3.5e-6 of the largest entry (bound 1e-4)."""
    c = SC.gpu_case(name)
    B, A = c["noise_pi"].shape
    g = torch.Generator().manual_seed(7)
    da, dl = torch.randn(B, A, generator=g), torch.randn(B, generator=g)
    ref = SC.actor_ref(c, da.numpy(), dl.numpy())
    head = _head(c)
    runs = []
    for _ in range(2):
        _clear(head)
        x = _t(c, "x").requires_grad_(True)
        actions, logp = head.action_log_prob(x, noise=_t(c, "noise_pi"))
        assert actions.shape == (B, A) and logp.shape == (B,) and actions.dtype == logp.dtype == torch.float32 and logp.requires_grad
        torch.autograd.backward([actions, logp], [da.to(DEV), dl.to(DEV)])
        torch.cuda.synchronize()
        grads = {n: p.grad.cpu() for n, p in head.named_parameters() if n.startswith("actor.")}
        grads["x"] = x.grad.cpu()
        runs.append(((actions.detach().cpu(), logp.detach().cpu()), grads))
    assert all(torch.equal(a, b) for a, b in zip(runs[0][0], runs[1][0])), "two runs differ in their bits (outputs)"
    assert all(torch.equal(runs[0][1][k], runs[1][1][k]) for k in runs[0][1]), "two runs differ in their bits (gradients)"
    assert all(p.grad is None for n, p in head.named_parameters() if not n.startswith("actor."))
    _check_values(name + " actions", runs[0][0][0], ref["actions"])
    _check_values(name + " log_prob", runs[0][0][1], ref["log_prob"])
    _check_grads(name, runs[0][1], ref["grad"])
    with torch.no_grad():
        quiet = head.action_log_prob(_t(c, "x"), noise=_t(c, "noise_pi"))
    assert torch.equal(quiet[0].cpu(), runs[0][0][0]) and torch.equal(quiet[1].cpu(), runs[0][0][1]) and not quiet[1].requires_grad
    det = head(_t(c, "x"), deterministic=True)
    assert not det.requires_grad
    _check_values(name + " deterministic", det, np.tanh(ref["mu"]))
    sampled = head(_t(c, "x"), noise=_t(c, "noise_pi"))
    assert torch.equal(sampled.cpu(), runs[0][0][0])


@pytest.mark.parametrize("name", ALL)
def test_q_values_forward_and_backward_against_the_restatement(name):
    """Both critics at (x, a_replay) with a random output gradient: q, d actions and every critic gradient; the features take none; the
    d-actions-only mode gives the bits of the full mode's d actions; target=True reads critic_target."""
    c = SC.gpu_case(name)
    B = c["x"].shape[0]
    g = torch.Generator().manual_seed(11)
    dq = torch.randn(2, B, generator=g)
    ref = SC.critic_ref(c, c["a_replay"], dq.numpy())
    head = _head(c)
    runs = []
    for mode in ("full", "full", "actions_only"):
        _clear(head)
        x = _t(c, "x").requires_grad_(True)
        a = _t(c, "a_replay").requires_grad_(True)
        q = head.q_values(x, a) if mode == "full" else SH.q_values(head.params(), x, a, param_grads=False)
        assert q.shape == (2, B) and q.dtype == torch.float32 and q.requires_grad
        q.backward(dq.to(DEV))
        torch.cuda.synchronize()
        assert x.grad is None, "the features enter the critics detached"
        grads = {n: p.grad.cpu() for n, p in head.named_parameters() if p.grad is not None}
        grads["actions"] = a.grad.cpu()
        runs.append((q.detach().cpu(), grads))
    assert torch.equal(runs[0][0], runs[1][0]) and all(torch.equal(runs[0][1][k], runs[1][1][k]) for k in runs[0][1]), "two runs differ in their bits"
    assert set(runs[2][1]) == {"actions"} and torch.equal(runs[2][1]["actions"], runs[0][1]["actions"]) and torch.equal(runs[2][0], runs[0][0])
    _check_values(name + " q", runs[0][0], ref["q"])
    _check_grads(name, runs[0][1], ref["grad"])
    with torch.no_grad():
        quiet = head.q_values(_t(c, "x"), _t(c, "a_replay"))
        qt = head.q_values(_t(c, "x"), _t(c, "a_replay"), target=True)
    assert torch.equal(quiet.cpu(), runs[0][0])
    rt = SC.critic_ref(c, c["a_replay"], dq.numpy(), prefix="critic_target")
    _check_values(name + " target q", qt, rt["q"])
    assert float(np.abs(rt["q"] - ref["q"]).max()) > 1e-2          # the targets are other numbers


@pytest.mark.parametrize("name", ALL)
def test_td_target_against_the_restatement_and_the_composition(name):
    """One launch against the restatement, and against action_log_prob -> q_values(target=True) -> torch arithmetic on the same GPU; the entropy
    coefficient as a float and as a pointer to its logarithm."""
    c = SC.gpu_case(name)
    ref = SC.gpu_reference(name)
    head = _head(c)
    xn, r, d, noise = _t(c, "x_next"), _t(c, "rewards"), _t(c, "dones"), _t(c, "noise_next")
    ent = float(ref["ent_coef"])
    log_ent = torch.tensor([math.log(ent)], dtype=torch.float32, device=DEV)
    by_float = head.td_target(xn, r, d, c["gamma"], ent_coef=ent, noise=noise)
    by_ptr = head.td_target(xn, r, d, c["gamma"], log_ent_coef=log_ent, noise=noise)
    again = head.td_target(xn, r, d, c["gamma"], ent_coef=ent, noise=noise)
    assert by_float.shape == (c["x"].shape[0],) and not by_float.requires_grad and torch.equal(by_float, again)
    _check_values(name + " target_q (float)", by_float, ref["target_q"])
    _check_values(name + " target_q (pointer)", by_ptr, ref["target_q"])
    with torch.no_grad():
        a2, lp2 = head.action_log_prob(xn, noise=noise)
        q2 = head.q_values(xn, a2, target=True)
        composed = r + (1 - d) * c["gamma"] * (torch.minimum(q2[0], q2[1]) - ent * lp2)
    _check_values(name + " target_q against the composition", by_float, composed.double().cpu().numpy())
    _check_values(name + " a'", a2, ref["a_next"])
    _check_values(name + " logp'", lp2, ref["log_prob_next"])
    if c["x"].shape[0] > 1:          # a done row is its reward, whatever the critics say
        assert torch.equal(by_float[1], r[1]) and float(d[1]) == 1.0 and float(d[0]) == 0.0


def _step(head, c, g=None):
    """The head's part of one gradient step in the reference's order (sac_mae.py:303-366) -> results as a nested dict of tensors."""
    check = g.check if g is not None else (lambda where="": None)
    _clear(head)
    out = {}
    x = _t(c, "x").requires_grad_(True)
    p = head.params()
    a_pi, logp = head.action_log_prob(x, noise=_t(c, "noise_pi"))                                     # :303
    check("after action_log_prob")
    log_ent = None
    if c["auto"]:
        log_ent = torch.tensor([c["log_ent_coef"]], dtype=torch.float32, device=DEV, requires_grad=True)
        ent_loss, ent = head.ent_coef_loss(log_ent, logp, c["target_entropy"])                       # :311-312
        assert ent_loss.dim() == 0 and ent.dim() == 0 and ent.is_cuda and not ent.requires_grad
        ent_loss.backward()                                                                          # :323
        check("after ent_coef_loss")
        out.update(ent_coef_loss=ent_loss.detach(), ent_coef=ent, grad_log_ent_coef=log_ent.grad)
    kw = _ent_kw(c, log_ent)
    target_q = head.td_target(_t(c, "x_next"), _t(c, "rewards"), _t(c, "dones"), c["gamma"], noise=_t(c, "noise_next"), **kw)      # :326-335
    check("after td_target")
    critic_loss = head.critic_loss(x, _t(c, "a_replay"), target_q)                                   # :339-342
    check("after critic_loss")
    critic_loss.backward()                                                                           # :348
    check("after critic_loss.backward")
    out["grad_critic"] = {n: gr.clone() for n, gr in _grads(head, "critic.").items()}
    assert all(p_.grad is None for n, p_ in head.named_parameters() if n.startswith("actor.")) and x.grad is None
    for n, p_ in head.named_parameters():                                                            # :347 of the next step
        if n.startswith("critic."):
            p_.grad = None
    q_pi = SH.q_values(p, x, a_pi, param_grads=False)                                                # :354
    actor_loss = SH.actor_loss_from(logp, q_pi, **kw)                                                # :355-356
    check("after actor_loss")
    actor_loss.backward()                                                                            # :361
    check("after actor_loss.backward")
    out["critic_untouched"] = all(p_.grad is None for n, p_ in head.named_parameters() if n.startswith("critic"))
    out["grad_actor"] = dict(_grads(head, "actor."))
    out["grad_x"] = x.grad
    head.polyak_update(c["tau"])                                                                     # :366
    check("after polyak_update")
    out["target"] = {n: p_.detach().clone() for n, p_ in head.named_parameters() if n.startswith("critic_target.")}
    out.update(a_pi=a_pi.detach(), log_prob=logp.detach(), target_q=target_q, critic_loss=critic_loss.detach(), q_pi=q_pi.detach(),
               actor_loss=actor_loss.detach())
    return out


def _check_step(what, c, out, ref, ref_grad, ref_target):
    for k in ("a_pi", "log_prob", "target_q", "critic_loss", "actor_loss"):
        _check_values(f"{what} {k}", out[k], ref[k])
    assert out["critic_loss"].dim() == 0 and out["actor_loss"].dim() == 0
    grads = dict(out["grad_critic"])
    grads.update(out["grad_actor"])
    grads["x"] = out["grad_x"]
    if c["auto"]:
        _check_values(f"{what} ent_coef_loss", out["ent_coef_loss"], ref["ent_coef_loss"])
        _check_values(f"{what} ent_coef", out["ent_coef"], ref["ent_coef"])
        grads["log_ent_coef"] = out["grad_log_ent_coef"]
    _check_grads(what, grads, ref_grad)
    assert out["critic_untouched"], "actor_loss left a gradient in the critic's parameters"
    assert set(out["target"]) == set(ref_target)
    for k, r in ref_target.items():
        _check_values(f"{what} {k} after polyak_update", out["target"][k], r)


@pytest.mark.parametrize("name", ALL)
def test_whole_step_against_the_restatement(name):
    """The three losses, every gradient the reference's optimizers see, and the Polyak update, in the reference's order."""
    c = SC.gpu_case(name)
    ref = SC.gpu_reference(name)
    head = _head(c)
    out = _step(head, c)
    torch.cuda.synchronize()
    _check_step(name, c, out, ref, ref["grad"], ref["target"])
    _check_values(name + " q_pi", out["q_pi"], ref["q_pi"])
    # the Polyak update moved the targets by tau of the distance, and nothing else
    before = {k: torch.from_numpy(np.asarray(v)) for k, v in c["params"].items()}
    for n, p in head.named_parameters():
        if not n.startswith("critic_target."):
            assert torch.equal(p.detach().cpu(), before[n]), n


@pytest.mark.parametrize("name", GOLDEN_CASES)
def test_whole_step_against_the_recorded_train_step(name):
    """The same against what the reference's own SAC_MAE.train computed (golden/sac_head_step.npz)."""
    c, rec = golden_case(name)
    out = _step(_head(c), c)
    torch.cuda.synchronize()
    ref = {k: rec[k] for k in ("a_pi", "log_prob", "target_q", "critic_loss", "actor_loss", "ent_coef")}
    if c["auto"]:
        ref["ent_coef_loss"] = rec["ent_coef_loss"]
    _check_step("golden " + name, c, out, ref, {k[len("grad/"):]: rec[k] for k in rec if k.startswith("grad/")},
                {k[len("target/"):]: rec[k] for k in rec if k.startswith("target/")})


@pytest.mark.parametrize("name", ["a64_b33", "mixed_b33", "amax_b3", "nohid_b33"])
def test_fused_losses_agree_with_the_same_losses_in_torch_on_the_nodes_outputs(name):
    """Each loss node against the reference's line written in torch on the same node outputs (values and the gradients that reach the leaves), and
    SACHead.actor_loss / critic_loss against the composed calls, bit for bit."""
    c = SC.gpu_case(name)
    head = _head(c)
    p = head.params()
    ent = 0.15
    target_q = head.td_target(_t(c, "x_next"), _t(c, "rewards"), _t(c, "dones"), c["gamma"], ent_coef=ent, noise=_t(c, "noise_next"))

    def run(fused):
        _clear(head)
        x = _t(c, "x").requires_grad_(True)
        log_ent = torch.tensor([c["log_ent_coef"]], dtype=torch.float32, device=DEV, requires_grad=True)
        a_pi, logp = head.action_log_prob(x, noise=_t(c, "noise_pi"))
        q_pi = SH.q_values(p, x, a_pi, param_grads=False)
        q_r = head.q_values(x, _t(c, "a_replay"))
        if fused:
            al = SH.actor_loss_from(logp, q_pi, ent_coef=ent)
            cl = SH.critic_loss_from(q_r, target_q)
            el, _ = SH.ent_coef_loss(log_ent, logp, c["target_entropy"])
        else:
            al = (ent * logp - torch.minimum(q_pi[0], q_pi[1])).mean()
            cl = 0.5 * sum(torch.nn.functional.mse_loss(q, target_q) for q in q_r)
            el = -(log_ent * (logp + c["target_entropy"]).detach()).mean()
        (0.5 * al + 2.0 * cl + 3.0 * el).backward()          # dloss other than 1 for each
        torch.cuda.synchronize()
        grads = {n: p_.grad.clone() for n, p_ in head.named_parameters() if p_.grad is not None}
        grads.update(x=x.grad, log_ent_coef=log_ent.grad)
        return (al.detach(), cl.detach(), el.detach()), grads
    (fa, fc, fe), fg = run(True)
    (ta, tc, te), tg = run(False)
    for what, f, t in (("actor_loss", fa, ta), ("critic_loss", fc, tc), ("ent_coef_loss", fe, te)):
        _check_values(f"{name} {what} fused against torch", f, t.double().cpu().numpy())
    _check_grads(name + " fused against torch", fg, {k: v.double().cpu().numpy() for k, v in tg.items()})
    # the module's one-call forms are the composed calls
    x = _t(c, "x")
    al, lp = head.actor_loss(x, ent_coef=ent, noise=_t(c, "noise_pi"))
    a_pi, logp = head.action_log_prob(x, noise=_t(c, "noise_pi"))
    assert torch.equal(al.detach(), SH.actor_loss_from(logp, SH.q_values(p, x, a_pi, param_grads=False), ent_coef=ent).detach()) and torch.equal(lp, logp.detach())
    assert not lp.requires_grad and al.requires_grad
    assert torch.equal(head.critic_loss(x, _t(c, "a_replay"), target_q).detach(), SH.critic_loss_from(head.q_values(x, _t(c, "a_replay")), target_q).detach())


@pytest.mark.parametrize("name", ["a64_b17", "mixed_b33", "amax_b65"])
def test_memory_contract(monkeypatch, name):
    """Every entry point under guarded, poisoned allocations at ragged-tile shapes: no write outside a buffer, no read of stale workspace, padding
    or outputs, and the bits of the unguarded run."""
    c = SC.gpu_case(name)
    params = {k: torch.from_numpy(np.asarray(v)).to(DEV) for k, v in c["params"].items()}
    head = _head(c)

    def work(g):
        with torch.no_grad():
            for n, p in head.named_parameters():
                p.copy_(params[n])          # the Polyak update of the run before is undone
        out = _step(head, c, g)
        out["deterministic"] = head(_t(c, "x"), deterministic=True)
        g.check("after the deterministic forward")
        return out
    counts = MG.run_contract(monkeypatch, work)
    assert counts[0] == counts[1] and counts[0][0] == 3          # three workspaces: the actor node's and the two critic nodes'


@pytest.mark.parametrize("name", ["a64_b17", "nohid_b3"])
def test_one_workspace_serves_the_actor_and_the_critics(name):
    """The header's promise at the C ABI: the actor and critic parts of one m3l_sac_ws_bytes workspace do not overlap.  One workspace handed to
    m3l_sac_actor_fwd and m3l_sac_critic_fwd, then to m3l_sac_critic_bwd (with grads) and m3l_sac_actor_bwd, gives every output and gradient
    the bits of the same four calls on two separate workspaces.  a64_b17: two row tiles, the second ragged; nohid_b3: no hidden layer, the
    smallest layouts, where an off-by-one in the critics' start lands inside the neighbour's part."""
    c = SC.gpu_case(name)
    p = _head(c).params()
    x, a, noise = _t(c, "x"), _t(c, "a_replay"), _t(c, "noise_pi")
    B, A = noise.shape
    arch = SH._arch(x.shape[1], p)
    af, cf = [SH._dev(t) for t in p.actor_flat()], [SH._dev(t) for t in p.critic_flat()]
    d = SH._desc(arch, actor=af, critic=cf)
    lib = L.lib()
    nbytes = lib.m3l_sac_ws_bytes(C.byref(d), B)
    g = torch.Generator().manual_seed(11)
    dq, da, dl = torch.randn(2, B, generator=g).to(DEV), torch.randn(B, A, generator=g).to(DEV), torch.randn(B, generator=g).to(DEV)

    def run(ws_actor, ws_critic):
        grads = [torch.zeros_like(t) for t in af + cf]
        gd = SH._desc(arch, actor=grads[:len(af)], critic=grads[len(af):])
        actions, logp, q = torch.empty(B, A, device=DEV), torch.empty(B, device=DEV), torch.empty(2, B, device=DEV)
        dactions, dx = torch.empty(B, A, device=DEV), torch.empty_like(x)
        L.check(lib.m3l_sac_actor_fwd(C.byref(d), B, L.ptr(x), L.ptr(noise), L.ptr(ws_actor), L.ptr(actions), L.ptr(logp), None), "m3l_sac_actor_fwd")
        L.check(lib.m3l_sac_critic_fwd(C.byref(d), B, L.ptr(x), L.ptr(a), L.ptr(ws_critic), L.ptr(q), None), "m3l_sac_critic_fwd")
        L.check(lib.m3l_sac_critic_bwd(C.byref(d), B, L.ptr(dq), L.ptr(ws_critic), L.ptr(dactions), C.byref(gd), None), "m3l_sac_critic_bwd")
        L.check(lib.m3l_sac_actor_bwd(C.byref(d), B, L.ptr(x), L.ptr(noise), L.ptr(da), L.ptr(dl), L.ptr(ws_actor), L.ptr(dx), C.byref(gd), None),
                "m3l_sac_actor_bwd")
        torch.cuda.synchronize()
        return [actions, logp, q, dactions, dx] + grads

    def ws():
        return torch.full((nbytes,), 0xFF, dtype=torch.uint8, device=DEV)          # NaN in every float: a stale read would show
    shared = ws()
    one, two = run(shared, shared), run(ws(), ws())
    assert all(bool(torch.isfinite(t).all()) for t in two) and any(bool(t.any()) for t in two[5:])
    for i, (got, want) in enumerate(zip(one, two)):
        assert torch.equal(got, want), f"tensor {i} of the shared-workspace run differs from the run on two workspaces"


@pytest.mark.parametrize("name", ["mixed_b33", "a256_b130"])
def test_no_grad_calls_take_no_workspace(monkeypatch, name):
    c = SC.gpu_case(name)
    head = _head(c)
    x, a, noise = _t(c, "x"), _t(c, "a_replay"), _t(c, "noise_pi")

    def no_grad(g):
        with torch.no_grad():
            out = list(head.action_log_prob(x, noise=noise)) + [head.q_values(x, a), head(x, noise=noise)]
        out.append(head.td_target(x, _t(c, "rewards"), _t(c, "dones"), 0.99, ent_coef=0.2, noise=noise))
        g.check("after the no_grad calls")
        return {"out": out}

    def grad(g):
        out = list(head.action_log_prob(x, noise=noise)) + [head.q_values(x, a)]
        g.check("after the grad-mode calls")
        return {"out": [t.detach() for t in out]}
    sized = []
    lib = L.lib()
    real = lib.m3l_sac_ws_bytes
    monkeypatch.setattr(lib, "m3l_sac_ws_bytes", lambda *args: sized.append(1) or real(*args))
    counts = MG.run_contract(monkeypatch, no_grad, need_ws=False)
    assert all(n_ws == 0 for n_ws, _ in counts) and not sized, (counts, len(sized))
    counts = MG.run_contract(monkeypatch, grad)
    assert all(n_ws == 2 for n_ws, _ in counts) and len(sized) == 6
    frozen = _head(c).requires_grad_(False)          # nothing requires a gradient: no workspace in grad mode either
    sized.clear()
    out = frozen.action_log_prob(x, noise=noise)
    q = frozen.q_values(x, a)
    assert not sized and not out[1].requires_grad and not q.requires_grad
    out = frozen.action_log_prob(x.clone().requires_grad_(True), noise=noise)          # the features alone do, for the actor
    q = frozen.q_values(x.clone().requires_grad_(True), a)                              # and never for the critics
    assert len(sized) == 1 and out[1].requires_grad and not q.requires_grad


def test_refusals_that_need_a_device():
    c = SC.gpu_case("a64_b3")
    head = _head(c)
    x, a, v = _t(c, "x"), _t(c, "a_replay"), _t(c, "rewards")
    for call in (lambda: head(x.cpu()), lambda: head.action_log_prob(x.cpu()), lambda: head.q_values(x, a.cpu()), lambda: head.q_values(x.cpu(), a),
                 lambda: head.td_target(x, v.cpu(), v, 0.99, ent_coef=0.1), lambda: head.td_target(x, v, v, 0.99, log_ent_coef=torch.zeros(1)),
                 lambda: head.critic_loss(x, a, v.cpu()), lambda: head.actor_loss(x.cpu(), ent_coef=0.1), lambda: head.ent_coef_loss(torch.zeros(1), v, -3.0),
                 lambda: head.action_log_prob(x, noise=torch.zeros(3, 3))):
        with pytest.raises(m3l_amd.M3LError):
            call()
    for call in (lambda: head.action_log_prob(x, noise=torch.zeros(2, 3, device=DEV)), lambda: head.q_values(x, a[:2]), lambda: head.q_values(x, a[:, :2]),
                 lambda: head.td_target(x, v[:2], v, 0.99, ent_coef=0.1), lambda: head.critic_loss(x, a, v[:2]), lambda: head.action_log_prob(x[:, :48]),
                 lambda: head.td_target(x, v, v, 0.99), lambda: head.td_target(x, v, v, 0.99, ent_coef=torch.zeros(1, device=DEV)),
                 lambda: SH.actor_loss_from(v[:2], torch.zeros(2, 3, device=DEV), ent_coef=0.1), lambda: SH.critic_loss_from(torch.zeros(3, 3, device=DEV), v)):
        with pytest.raises(ValueError):
            call()
    # the C ABI refuses what the header excludes, with the reason, and writes nothing
    lib = L.lib()
    p = head.params()
    arch = SH._arch(64, p)
    q = torch.full((2, 3), 7.0, device=DEV)
    for change, why in ((dict(features=40), "multiple of 16"), (dict(actions=65), "1 <= A <= 64"), (dict(n_qf=4), "hidden layers"), (dict(B=0), "B >= 1")):
        d = SH._desc(arch, actor=p.actor_flat(), critic=p.critic_flat())
        B = change.pop("B", 3)
        for k, val in change.items():
            setattr(d, k, val)
        assert lib.m3l_sac_critic_fwd(C.byref(d), B, L.ptr(x), L.ptr(a), None, L.ptr(q), None) != 0 and why in L.last_error(), L.last_error()
        assert lib.m3l_sac_actor_fwd(C.byref(d), B, L.ptr(x), None, None, L.ptr(a), L.ptr(v), None) != 0 and why in L.last_error()
    d = SH._desc(arch, actor=p.actor_flat())          # no critic pointers
    assert lib.m3l_sac_critic_fwd(C.byref(d), 3, L.ptr(x), L.ptr(a), None, L.ptr(q), None) != 0 and "null" in L.last_error()
    assert lib.m3l_sac_critic_loss_fwd(L.ptr(q), L.ptr(v), 0, L.ptr(v), L.ptr(q), None) != 0
    torch.cuda.synchronize()
    assert bool((q == 7.0).all())


def test_end_to_end_extractor_head_actor_loss():
    """MAEExtractor -> SACHead.actor_loss(...).backward() against the same extractor with the restatement's head in float32 torch on the GPU: loss
    and actor gradients within the bounds above, the encoder's parameter gradients within the extractor tests' float32 gradient bound
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
    c = SC.make_inputs(SC.ARCHS["a64"], B, False, True, seed=77)
    head = _head(c)
    noise = torch.randn(B, A, generator=g).to(DEV)
    ent = 0.2

    def grads_of():
        out = {"head." + n: p.grad.clone() for n, p in head.named_parameters() if p.grad is not None}
        out.update({"ext." + n: p.grad.clone() for n, p in ext.named_parameters() if p.grad is not None})
        for p in list(head.parameters()) + list(ext.parameters()):
            p.grad = None
        return out

    loss, logp = head.actor_loss(ext(obs), ent_coef=ent, noise=noise)
    loss.backward()
    got = grads_of()
    P = {n: p for n, p in head.named_parameters()}
    feat = ext(obs)
    o = SC.actor_forward(P, feat, noise, stable=True)
    q, pre_q = SC.critic_forward(P, "critic", feat, o["actions"])
    want_loss = (ent * o["log_prob"] - torch.minimum(q[0], q[1])).mean()
    want_loss.backward()
    want = {k: v for k, v in grads_of().items() if not k.startswith("head.critic")}          # the HIP head leaves the critic's parameters alone
    torch.cuda.synchronize()
    pres = torch.cat([p.detach().flatten() for p in o["pre"] + pre_q])
    assert float(pres.abs().min()) > 1e-4 and float((q[0] - q[1]).detach().abs().min()) > 1e-3, "an input sits on a gate or a tie"
    _check_values("end to end loss", loss.detach(), float(want_loss.detach()))
    _check_values("end to end log_prob", logp, o["log_prob"].detach().double().cpu().numpy())
    assert set(got) == set(want) and any(k.startswith("ext.mae.") or k.startswith("ext.vit_layer.") for k in got) and not any(k.startswith("head.critic") for k in got)
    for k in want:
        gmax = float(want[k].abs().max())
        err = float((got[k] - want[k]).abs().max())
        bound = GRAD_TOL * gmax if k.startswith("head.") else 3e-3 * gmax + 1e-7
        assert err <= bound, (k, err, bound)
