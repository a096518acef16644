"""GPU checks of the TD3 head (m3l_td3_*, m3l_amd.TD3Head, m3l_amd/td3.py).

Yardstick: the float64 restatement of tests/td3_cases.py, which test_td3_cpu.py pins to a loop-written version and a hand-computed example.
Every input satisfies the conditions test_td3_cpu.py asserts: every ReLU pre-activation at least GATE_MARGIN from 0, the two smallest critics
at least TIE_MARGIN apart where "min" takes a gradient, no entry within CLAMP_MARGIN of a clamp's edge and entries on both sides of each, so
the gates, the chosen critic and the clamped entries are the same in float32 and float64.  Bounds, the other heads': values within 1e-4 of
max(1, |ref|), every gradient tensor within 1e-4 of its largest float64 entry.  The critic loss is compared bit for bit with twice
SACEnsembleHead's, q_values bit for bit with SACEnsembleHead's.  Measured on an MI355X (EXPERIMENTS.md 5.34): values within 1.7e-6, gradients
within 1.4e-6."""
import ctypes as C

import numpy as np
import pytest
import torch

import m3l_amd
import memguard as MG
import td3_cases as TC
from m3l_amd import _lib as L
from m3l_amd import td3 as T3
from test_sac_head_gpu import _check_grads, _check_values, _clear

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ALL = list(TC.CASES)
CONTRACT = ["amax_n3_b1", "f16a7_n2_b17", TC.ANCHOR]          # B = 1, B = 17, the step's shape


def _head(c):
    Fd, pi, qf, A = c["arch"]
    head = m3l_amd.TD3Head(Fd, A, net_arch=dict(pi=list(pi), qf=list(qf)), n_critics=c["n_critics"])
    head.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in c["params"].items()}, strict=True)
    return head.to(DEV)


def _ens(c):
    """A SACEnsembleHead with the case's critics and target critics (its own actor is not used)."""
    Fd, pi, qf, A = c["arch"]
    head = m3l_amd.SACEnsembleHead(Fd, A, net_arch=dict(pi=list(pi), qf=list(qf)), n_critics=c["n_critics"])
    for part in ("critic", "critic_target"):
        getattr(head, part).load_state_dict({k[len(part) + 1:]: torch.from_numpy(np.asarray(v)) for k, v in c["params"].items() if k.startswith(part + ".")})
    return head.to(DEV)


def _t(c, k):
    return torch.from_numpy(c[k]).to(DEV)


def _grads(head):
    return {n: p.grad.clone() for n, p in head.named_parameters() if p.grad is not None}


def _same(a, b):
    return set(a) == set(b) and all(torch.equal(a[k], b[k]) for k in a)


@pytest.mark.parametrize("name", ALL)
def test_actor_forward_and_backward_against_the_restatement(name):
    """actions in the three noise modes with a random output gradient: the actions, dx and every actor gradient; the target actor takes none;
    two runs give equal bits; the no_grad call gives the same bits; sigma = 0 and a noise of zeros give the deterministic bits."""
    c = TC.case(name)
    B, A = c["noise_pi"].shape
    da = torch.randn(B, A, generator=torch.Generator().manual_seed(5))
    head = _head(c)
    noise = _t(c, "noise_pi")
    det = None
    for mode, (sigma, clip) in TC.MODES.items():
        ref = TC.actions_ref(c, mode, da.numpy())
        runs = []
        for _ in range(2):
            _clear(head)
            x = _t(c, "x").requires_grad_(True)
            a = head.actions(x, noise=noise, noise_std=sigma, noise_clip=clip)
            assert a.shape == (B, A) and a.dtype == torch.float32 and a.requires_grad
            a.backward(da.to(DEV))
            torch.cuda.synchronize()
            g = _grads(head)
            g["x"] = x.grad.clone()
            runs.append((a.detach().clone(), g))
        assert torch.equal(runs[0][0], runs[1][0]) and _same(runs[0][1], runs[1][1]), f"{mode}: two runs differ in their bits"
        assert not any(k.startswith(("actor_target", "critic")) for k in runs[0][1])
        _check_values(f"{name} actions {mode}", runs[0][0], ref["actions"])
        _check_grads(f"{name} actions {mode}", runs[0][1], ref["grad"])
        quiet = head(_t(c, "x"), noise=noise, noise_std=sigma, noise_clip=clip)
        assert torch.equal(quiet, runs[0][0]) and not quiet.requires_grad
        assert float(runs[0][0].abs().max()) <= 1.0
        if mode == "det":
            det = runs[0][0]
    with torch.no_grad():
        assert torch.equal(head.actions(_t(c, "x")), det) and torch.equal(head.actions(_t(c, "x"), noise=noise, noise_std=0.0, noise_clip=0.5), det)
        assert torch.equal(head.actions(_t(c, "x"), noise=torch.zeros_like(noise), noise_std=0.6, noise_clip=0.5), det)
        assert torch.equal(head.actions(_t(c, "x"), noise=torch.zeros_like(noise), noise_std=0.6), det)


def _swapped(c):
    """The case's head with the two actors exchanged: its `forward` runs the case's target actor."""
    sd = {}
    for k, v in c["params"].items():
        k2 = k.replace("actor_target.", "actor.") if k.startswith("actor_target.") else k.replace("actor.", "actor_target.") if k.startswith("actor.") else k
        sd[k2] = torch.from_numpy(np.asarray(v))
    Fd, pi, qf, A = c["arch"]
    head = m3l_amd.TD3Head(Fd, A, net_arch=dict(pi=list(pi), qf=list(qf)), n_critics=c["n_critics"])
    head.load_state_dict(sd, strict=True)
    return head.to(DEV)


@pytest.mark.parametrize("name", ALL)
def test_td_target_against_the_restatement(name):
    """One launch per call: the three noise modes with the target actor and with the online one (their weights differ), gamma as a number and
    as one discount per row; a constant discounts tensor gives the number's bits; a done row is its reward; two calls give equal bits; the
    composition forward -> q_values(target=True) -> min on the same GPU agrees within the bound."""
    c, ref = TC.case(name), TC.reference(name)
    B = c["x"].shape[0]
    head, swapped = _head(c), _swapped(c)
    xn, r, d, disc = _t(c, "x_next"), _t(c, "rewards"), _t(c, "dones"), _t(c, "discounts")
    assert not torch.equal(head.actor.mu[0].weight, head.actor_target.mu[0].weight)
    for online in (False, True):
        noise = _t(c, "noise_next_online" if online else "noise_next")
        for mode, (sigma, clip) in TC.MODES.items():
            kw = dict(noise=noise, target_policy_noise=sigma, target_noise_clip=clip, use_actor_target=not online)
            got = head.td_target(xn, r, d, c["gamma"], **kw)
            rows = head.td_target(xn, r, d, disc.reshape(B, 1), **kw)
            assert got.shape == (B,) and not got.requires_grad and torch.equal(got, head.td_target(xn, r, d, c["gamma"], **kw))
            what = f"{name} target_q {mode} {'online' if online else 'target'} actor"
            _check_values(what, got, TC.target_ref(c, ref, mode, c["gamma"], online))
            _check_values(what + " (per-row discounts)", rows, TC.target_ref(c, ref, mode, c["discounts"], online))
            const = torch.full((B,), c["gamma"], dtype=torch.float32, device=DEV)
            assert torch.equal(head.td_target(xn, r, d, const, **kw), got)
            if B > 1:
                assert torch.equal(got[1], r[1]) and float(d[1]) == 1.0 and float(d[0]) == 0.0
            actor = head if online else swapped
            with torch.no_grad():
                a2 = actor(xn, noise=noise, noise_std=sigma, noise_clip=clip)
                composed = r + (1 - d) * c["gamma"] * head.q_values(xn, a2, target=True).min(dim=0)[0]
            _check_values(what + " against the composition", got, composed.double().cpu().numpy())
        assert torch.equal(head.td_target(xn, r, d, c["gamma"], noise=noise, target_policy_noise=0.0, use_actor_target=not online),
                           head.td_target(xn, r, d, c["gamma"], noise=None, target_policy_noise=0.0, target_noise_clip=None, use_actor_target=not online))
    drawn = head.td_target(xn, r, d, c["gamma"])          # noise=None: a draw on the device, SB3's defaults
    assert drawn.shape == (B,) and bool(torch.isfinite(drawn).all())


@pytest.mark.parametrize("name", ALL)
def test_losses_and_their_gradients(name, monkeypatch):
    """critic_loss with and without weights: the loss and every gradient bit for bit twice SACEnsembleHead's on the same critics, td_abs its
    bits, and all three against the restatement.  actor_loss for "first", "min" and "mean" (and "min" on clipped noisy actions, DrQ-v2's): the
    loss, dx and the actor's gradients against the restatement, nothing in the critics or the target actor; "first" launches one critic."""
    c = TC.case(name)
    N = c["n_critics"]
    head, ens = _head(c), _ens(c)
    x, a, w = _t(c, "x"), _t(c, "a_replay"), _t(c, "weights")
    target_q = head.td_target(_t(c, "x_next"), _t(c, "rewards"), _t(c, "dones"), c["gamma"], noise=_t(c, "noise_next"), target_policy_noise=TC.SIGMA,
                              target_noise_clip=TC.CLIP)
    t64 = target_q.double().cpu().numpy()
    for what, weights in (("plain", None), ("weighted", w)):
        res = {}
        for label, h in (("td3", head), ("ens", ens)):
            _clear(h)
            loss, td = h.critic_loss(x, a, target_q, weights=weights, return_td_errors=True)
            assert loss.dim() == 0 and td.shape == target_q.shape and not td.requires_grad
            (3.0 * loss).backward()
            torch.cuda.synchronize()
            res[label] = (loss.detach(), td, _grads(h))
        assert torch.equal(res["td3"][0], 2.0 * res["ens"][0]), f"{what}: the loss is not twice the ensemble's, bit for bit"
        assert torch.equal(res["td3"][1], res["ens"][1])
        assert set(res["td3"][2]) == set(res["ens"][2]) == set(TC.EC.critic_names(c["arch"], N))
        for k, g in res["td3"][2].items():
            assert torch.equal(g, 2.0 * res["ens"][2][k]), f"{what}: {k} is not twice the ensemble's gradient, bit for bit"
        ref = TC.critic_loss_ref(c, t64, None if weights is None else c["weights"])
        _check_values(f"{name} critic_loss {what}", res["td3"][0], ref["loss"])
        _check_values(f"{name} td_abs {what}", res["td3"][1], ref["td_abs"])
        _check_grads(f"{name} critic_loss {what}", res["td3"][2], {k: 3.0 * v for k, v in ref["grad"].items()})
        _clear(head)
        assert torch.equal(head.critic_loss(x, a, target_q, weights=weights), res["td3"][0])
    launched = []
    lib = L.lib()
    real = lib.m3l_sac_ens_critic_fwd
    monkeypatch.setattr(lib, "m3l_sac_ens_critic_fwd", lambda d, *rest: launched.append(int(d._obj.n_critics)) or real(d, *rest))
    for reduce, mode in (("first", "det"), ("min", "det"), ("mean", "det"), ("min", "clip")):
        sigma, clip = TC.MODES[mode]
        runs = []
        for _ in range(2):
            _clear(head)
            launched.clear()
            xg = x.clone().requires_grad_(True)
            loss = head.actor_loss(xg, q_reduce=reduce, noise=_t(c, "noise_pi"), noise_std=sigma, noise_clip=clip)
            assert loss.dim() == 0 and launched == [1 if reduce == "first" else N], (reduce, launched)
            (2.0 * loss).backward()
            torch.cuda.synchronize()
            g = _grads(head)
            g["x"] = xg.grad.clone()
            runs.append((loss.detach(), g))
        assert torch.equal(runs[0][0], runs[1][0]) and _same(runs[0][1], runs[1][1]), "two runs differ in their bits"
        assert not any(k.startswith(("critic", "actor_target")) for k in runs[0][1]), "actor_loss left a gradient outside the actor"
        ref = TC.actor_loss_ref(c, reduce, mode)
        _check_values(f"{name} actor_loss {reduce} {mode}", runs[0][0], ref["loss"])
        _check_grads(f"{name} actor_loss {reduce} {mode}", runs[0][1], {k: 2.0 * v for k, v in ref["grad"].items()})


@pytest.mark.parametrize("name", ALL)
def test_q_values_have_the_ensembles_bits(name):
    c = TC.case(name)
    head, ens = _head(c), _ens(c)
    x, a = _t(c, "x"), _t(c, "a_replay")
    dq = torch.randn(c["n_critics"], x.shape[0], generator=torch.Generator().manual_seed(3)).to(DEV)
    out = {}
    for label, h in (("td3", head), ("ens", ens)):
        _clear(h)
        ag = a.clone().requires_grad_(True)
        q = h.q_values(x, ag)
        q.backward(dq)
        with torch.no_grad():
            qt = h.q_values(x, a, target=True)
        torch.cuda.synchronize()
        out[label] = dict(q=q.detach(), qt=qt, da=ag.grad, **_grads(h))
    assert not MG.differing(out["td3"], out["ens"])
    _check_values(name + " q", out["td3"]["q"], TC.reference(name)["q_replay"])


def _step(head, c, g=MG.NoGuard()):
    """One gradient step of the head: target -> critic loss and backward -> actor loss and backward -> Polyak on both nets."""
    _clear(head)
    x = _t(c, "x").requires_grad_(True)
    target_q = head.td_target(_t(c, "x_next"), _t(c, "rewards"), _t(c, "dones"), c["gamma"], noise=_t(c, "noise_next"), target_policy_noise=TC.SIGMA,
                              target_noise_clip=TC.CLIP)
    g.check("after td_target")
    closs = head.critic_loss(x, _t(c, "a_replay"), target_q)
    closs.backward()
    g.check("after critic_loss.backward")
    aloss = head.actor_loss(x, q_reduce="first")
    aloss.backward()
    g.check("after actor_loss.backward")
    grad = _grads(head)
    grad["x"] = x.grad.clone()
    head.polyak_update(c["tau"])
    g.check("after polyak_update")
    target = {n: p.detach().clone() for n, p in head.named_parameters() if "_target." in n}
    return dict(target_q=target_q, critic_loss=closs.detach(), actor_loss=aloss.detach(), grad=grad, target=target)


@pytest.mark.parametrize("name", [TC.ANCHOR, "nohid_n10_b3"])
def test_the_whole_step_against_the_restatement(name):
    c = TC.case(name)
    ref = TC.step_ref(c)
    got, again = _step(_head(c), c), _step(_head(c), c)
    torch.cuda.synchronize()
    assert not MG.differing(got, again), "two runs differ in their bits"
    for k in ("target_q", "critic_loss", "actor_loss"):
        _check_values(f"{name} step {k}", got[k], ref[k])
    _check_grads(name + " step", got["grad"], ref["grad"])
    assert set(got["target"]) == set(ref["target"])
    for k, r in ref["target"].items():
        _check_values(f"{name} {k} after polyak_update", got["target"][k], r)
        assert not torch.equal(got["target"][k].cpu(), torch.from_numpy(c["params"][k])), k


def _contract(head, c, g):
    """Every new entry point once: the actor both ways in a noisy mode, the target with per-row discounts and the online actor, the critic loss
    with weights, the three actor losses, and the step."""
    _clear(head)
    x = _t(c, "x").requires_grad_(True)
    a = head.actions(x, noise=_t(c, "noise_pi"), noise_std=TC.SIGMA, noise_clip=TC.CLIP)
    g.check("after actions")
    a.backward(torch.ones_like(a))
    g.check("after actions.backward")
    out = dict(actions=a.detach(), grad_actions=_grads(head), dx=x.grad.clone())
    out["rows"] = head.td_target(_t(c, "x_next"), _t(c, "rewards"), _t(c, "dones"), _t(c, "discounts"), noise=_t(c, "noise_next_online"),
                                 target_policy_noise=TC.SIGMA, target_noise_clip=None, use_actor_target=False)
    g.check("after td_target")
    _clear(head)
    loss, td = head.critic_loss(x, _t(c, "a_replay"), out["rows"], weights=_t(c, "weights"), return_td_errors=True)
    loss.backward()
    g.check("after the weighted critic_loss")
    out.update(critic_loss=loss.detach(), td=td, grad_critic=_grads(head))
    for reduce in ("first", "min", "mean"):
        _clear(head)
        al = head.actor_loss(x, q_reduce=reduce, noise=_t(c, "noise_pi"), noise_std=TC.SIGMA)
        al.backward()
        g.check(f"after actor_loss {reduce}")
        out["actor_" + reduce] = dict(loss=al.detach(), grad=_grads(head))
    out["step"] = _step(head, c, g)
    return out


@pytest.mark.parametrize("name", CONTRACT)
def test_memory_contract(monkeypatch, name):
    """Every new entry point under guarded, poisoned allocations: no write outside a buffer, no read of stale workspace, padding or outputs, and
    the bits of the unguarded run."""
    c = TC.case(name)
    params = {k: torch.from_numpy(np.asarray(v)).to(DEV) for k, v in c["params"].items()}
    head = _head(c)

    def work(g):
        with torch.no_grad():
            for n, p in head.named_parameters():
                p.copy_(params[n])          # the Polyak update of the run before is undone
        return _contract(head, c, g)
    counts = MG.run_contract(monkeypatch, work)
    # workspaces: the actor node; the critic node of the critic loss; actor + critic node per actor loss (3); the step's critic loss and actor loss
    assert counts[0] == counts[1] and counts[0][0] == 1 + 1 + 6 + 3, counts


def test_no_grad_calls_take_no_workspace(monkeypatch):
    c = TC.case("f16a7_n2_b17")
    head = _head(c)
    x, a, noise = _t(c, "x"), _t(c, "a_replay"), _t(c, "noise_pi")
    sized = []
    lib = L.lib()
    for fn in ("m3l_td3_ws_bytes", "m3l_sac_ens_ws_bytes"):
        monkeypatch.setattr(lib, fn, (lambda real: lambda *args: sized.append(1) or real(*args))(getattr(lib, fn)))

    def no_grad(g):
        with torch.no_grad():
            out = [head(x, noise=noise, noise_std=0.3, noise_clip=0.5), head.actions(x), head.q_values(x, a), head.q_values(x, a, target=True)]
        out.append(head.td_target(x, _t(c, "rewards"), _t(c, "dones"), 0.99, noise=noise))
        g.check("after the no_grad calls")
        return {"out": out}
    counts = MG.run_contract(monkeypatch, no_grad, need_ws=False)
    assert all(n_ws == 0 for n_ws, _ in counts) and not sized, (counts, len(sized))
    frozen = _head(c).requires_grad_(False)          # nothing requires a gradient: no workspace in grad mode either
    assert not frozen.actions(x).requires_grad and not sized
    assert frozen.actions(x.clone().requires_grad_(True)).requires_grad and len(sized) == 1
    assert head.actions(x).requires_grad and len(sized) == 2


def test_refusals_that_need_a_device():
    c = TC.case("a64_n3_b3")
    head = _head(c)
    x, a, v, noise = _t(c, "x"), _t(c, "a_replay"), _t(c, "rewards"), _t(c, "noise_pi")
    for call in (lambda: head(x.cpu()), lambda: head.actions(x, noise=noise.cpu(), noise_std=0.1), lambda: head.q_values(x, a.cpu()),
                 lambda: head.q_values(x.cpu(), a), lambda: head.td_target(x, v.cpu(), v, 0.99), lambda: head.td_target(x.cpu(), v, v, 0.99),
                 lambda: head.critic_loss(x, a, v.cpu()), lambda: head.critic_loss(x, a, v, weights=v.cpu()), lambda: head.actor_loss(x.cpu()),
                 lambda: T3.actor_loss_from(torch.zeros(1, 3)), lambda: m3l_amd.TD3Head(64, 3, net_arch=[64, 64])(x)):
        with pytest.raises(m3l_amd.M3LError):
            call()
    dev = lambda *s, **k: torch.zeros(*s, device=DEV, **k)      # noqa: E731
    for call in (lambda: head.actions(x, noise=noise[:2], noise_std=0.1), lambda: head.actions(x, noise=noise[:, :2], noise_std=0.1),
                 lambda: head.actions(x, noise=noise, noise_std=-0.1), lambda: head.actions(x, noise=noise, noise_std=float("nan")),
                 lambda: head.actions(x, noise=noise, noise_std=0.1, noise_clip=0.0), lambda: head.actions(x, noise=noise, noise_std=0.1, noise_clip=-1.0),
                 lambda: head.td_target(x, v, v, 0.99, target_policy_noise=-1.0), lambda: head.td_target(x, v, v, 0.99, target_policy_noise=float("inf")),
                 lambda: head.td_target(x, v, v, 0.99, target_noise_clip=0.0), lambda: head.td_target(x, v, v, 0.99, noise=noise[:2]),
                 lambda: head.td_target(x, v[:2], v, 0.99), lambda: head.td_target(x, v, v, dev(2)), lambda: head.q_values(x, a[:2]),
                 lambda: head.critic_loss(x, a, v[:2]), lambda: head.critic_loss(x, a, v, weights=v[:2]), lambda: head.actor_loss(x, q_reduce="max"),
                 lambda: T3.actor_loss_from(dev(3, 3), "first"), lambda: T3.critic_loss_from(dev(11, 3), v), lambda: head.actions(dev(3, 48))):
        with pytest.raises(ValueError):
            call()
    # the C ABI refuses what the header excludes, with the reason, and writes nothing
    lib = L.lib()
    p = head.params()
    arch = T3._arch(64, p)
    out = torch.full((3, 3), 7.0, device=DEV)
    make = lambda: T3._desc(arch, 3, actor=p.actor_flat(), critic=p.critic_flat(True))      # noqa: E731
    for change, why in ((dict(n_critics=0), "n_critics"), (dict(n_critics=11), "n_critics"), (dict(features=40), "multiple of 16"), (dict(n_pi=4), "hidden layers"),
                        (dict(actions=65), "actions"), (dict(B=0), "B >= 1"), (dict(sigma=-1.0), "sigma"), (dict(sigma=float("nan")), "sigma"),
                        (dict(mu_weight=None), "null")):
        d = make()
        B, sigma = change.pop("B", 3), change.pop("sigma", 0.2)
        for k, val in change.items():
            setattr(d, k, val)
        assert lib.m3l_td3_actor_fwd(C.byref(d), B, L.ptr(x), L.ptr(noise), sigma, 0.5, None, L.ptr(out), None) != 0 and why in L.last_error(), L.last_error()
        assert lib.m3l_td3_td_target(C.byref(d), B, L.ptr(x), L.ptr(noise), sigma, 0.5, L.ptr(v), L.ptr(v), None, 0.99, L.ptr(out), None) != 0
        assert why in L.last_error(), L.last_error()
    d = make()
    assert lib.m3l_td3_actor_fwd(C.byref(d), 3, None, None, 0.0, 0.0, None, L.ptr(out), None) != 0 and "null" in L.last_error()
    assert lib.m3l_td3_actor_bwd(C.byref(d), 3, L.ptr(x), L.ptr(out), None, L.ptr(out), C.byref(d), None) != 0 and "null" in L.last_error()
    assert lib.m3l_td3_actor_bwd(C.byref(d), 3, L.ptr(x), L.ptr(out), L.ptr(x), L.ptr(out), None, None) != 0 and "gradient descriptor" in L.last_error()
    assert lib.m3l_td3_td_target(C.byref(T3._desc(arch, 3, actor=p.actor_flat())), 3, L.ptr(x), None, 0.0, 0.0, L.ptr(v), L.ptr(v), None, 0.99, L.ptr(out), None) != 0
    assert lib.m3l_td3_critic_loss_fwd(L.ptr(out), L.ptr(v), None, 11, 3, L.ptr(out), L.ptr(out), None, None) != 0
    assert lib.m3l_td3_actor_loss_fwd(L.ptr(out), 3, 3, 2, L.ptr(out), L.ptr(out), None) != 0 and "reduce" in L.last_error()
    assert lib.m3l_td3_actor_loss_fwd(L.ptr(out), 0, 3, 0, L.ptr(out), L.ptr(out), None) != 0
    torch.cuda.synchronize()
    assert bool((out == 7.0).all())
