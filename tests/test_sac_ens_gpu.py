"""GPU checks of the SAC critic ensemble (m3l_sac_ens_*, m3l_amd.SACEnsembleHead, m3l_amd/sac_ensemble.py).

Yardstick: the float64 restatement of tests/sac_ens_cases.py, which test_sac_ens_cpu.py pins to sac_cases' own step at N = 2 (and that to the
step recorded from the reference's `SAC_MAE.train`).  Every input satisfies the conditions test_sac_ens_cpu.py asserts: every ReLU
pre-activation of all N critics at least GATE_MARGIN from 0, the two smallest values at least TIE_MARGIN apart wherever a minimum is taken, so
the gates and the chosen critic are the same in float32 and float64.  Bounds, the existing head's (test_sac_head_gpu.py): values within 1e-4 of
max(1, |ref|), every gradient tensor within 1e-4 of its largest float64 entry.  Measured on an MI355X (EXPERIMENTS.md 5.31): values within
6.0e-6, gradients within 3.1e-6; at N = 2 every output and gradient has SACHead's bits."""
import ctypes as C

import numpy as np
import pytest
import torch

import m3l_amd
import memguard as MG
import sac_cases as SC
import sac_ens_cases as EC
from m3l_amd import _lib as L
from m3l_amd import sac as SH
from m3l_amd import sac_ensemble as SE
from test_sac_head_gpu import _check_grads, _check_values, _clear

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ALL = list(EC.CASES)
CONTRACT = ["a64_n3_b17", "mixed_n5_b1", "amax_n3_b17"]
INT_MAX = 2 ** 31 - 1


def _head(c, cls=None):
    Fd, pi, qf, A = c["arch"]
    kw = dict(n_critics=c["n_critics"]) if cls is None else {}
    head = (cls or m3l_amd.SACEnsembleHead)(Fd, A, net_arch=dict(pi=list(pi), qf=list(qf)), **kw)
    head.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in c["params"].items()}, strict=True)
    return head.to(DEV)


def _t(c, k):
    return torch.from_numpy(c[k]).to(DEV)


def _sub(s):
    return None if s is None else torch.tensor(s, dtype=torch.int32, device=DEV)


def _log_ent(c):
    return torch.tensor([c["log_ent_coef"]], dtype=torch.float32, device=DEV)


def _same(a, b):
    return set(a) == set(b) and all(torch.equal(a[k], b[k]) for k in a)


@pytest.mark.parametrize("name", ALL)
def test_q_values_forward_and_backward_against_the_restatement(name):
    """All N critics at (x, a_replay) with a random output gradient: q (N, B), d actions (the chain over the critics) and every critic gradient
    (the grouped launches); the features take none; two runs give equal bits; the d-actions-only mode and the no_grad call give the same bits;
    target=True reads critic_target."""
    c = EC.case(name)
    N, B = c["n_critics"], c["x"].shape[0]
    dq = torch.randn(N, B, generator=torch.Generator().manual_seed(11))
    ref = EC.q_ref(c, c["a_replay"], dq.numpy())
    head = _head(c)
    runs = []
    for mode in ("full", "full", "actions_only"):
        _clear(head)
        x = _t(c, "x").requires_grad_(True)
        a = _t(c, "a_replay").requires_grad_(True)
        q = head.q_values(x, a) if mode == "full" else SE.q_values(head.params(), x, a, param_grads=False)
        assert q.shape == (N, B) and q.dtype == torch.float32 and q.requires_grad
        q.backward(dq.to(DEV))
        torch.cuda.synchronize()
        assert x.grad is None, "the features enter the critics detached"
        grads = {n: p.grad.cpu() for n, p in head.named_parameters() if p.grad is not None}
        grads["actions"] = a.grad.cpu()
        runs.append((q.detach().cpu(), grads))
    assert torch.equal(runs[0][0], runs[1][0]) and _same(runs[0][1], runs[1][1]), "two runs differ in their bits"
    assert set(runs[2][1]) == {"actions"} and torch.equal(runs[2][1]["actions"], runs[0][1]["actions"]) and torch.equal(runs[2][0], runs[0][0])
    _check_values(name + " q", runs[0][0], ref["q"])
    _check_grads(name, runs[0][1], ref["grad"])
    with torch.no_grad():
        quiet = head.q_values(_t(c, "x"), _t(c, "a_replay"))
        qt = head.q_values(_t(c, "x"), _t(c, "a_replay"), target=True)
    assert torch.equal(quiet.cpu(), runs[0][0]) and not quiet.requires_grad
    _check_values(name + " target q", qt, EC.q_ref(c, c["a_replay"], dq.numpy(), prefix="critic_target")["q"])


@pytest.mark.parametrize("name", ALL)
def test_td_target_for_every_subset_against_the_restatement(name):
    """One launch per call: every subset of the case, gamma as a number and as one discount per row, the entropy coefficient as a number and as
    a pointer to its logarithm; a done row is its reward; two calls give equal bits."""
    c, ref = EC.case(name), EC.reference(name)
    N, B = c["n_critics"], c["x"].shape[0]
    head = _head(c)
    xn, r, d, noise, disc = _t(c, "x_next"), _t(c, "rewards"), _t(c, "dones"), _t(c, "noise_next"), _t(c, "discounts")
    ent = EC.ent_of(c)
    for sub in EC.subsets(N):
        s = _sub(sub)
        by_float = head.td_target(xn, r, d, c["gamma"], ent_coef=ent, noise=noise, subset=s)
        by_ptr = head.td_target(xn, r, d, c["gamma"], log_ent_coef=_log_ent(c), noise=noise, subset=s)
        rows = head.td_target(xn, r, d, disc.reshape(B, 1), ent_coef=ent, noise=noise, subset=s)
        again = head.td_target(xn, r, d, c["gamma"], ent_coef=ent, noise=noise, subset=s)
        assert by_float.shape == (B,) and not by_float.requires_grad and torch.equal(by_float, again)
        _check_values(f"{name} target_q {sub} (float)", by_float, EC.target_ref(c, ref, sub, c["gamma"], ent))
        _check_values(f"{name} target_q {sub} (pointer)", by_ptr, EC.target_ref(c, ref, sub, c["gamma"], ent))
        _check_values(f"{name} target_q {sub} (per-row discounts)", rows, EC.target_ref(c, ref, sub, c["discounts"], ent))
        if B > 1:
            assert torch.equal(by_float[1], r[1]) and float(d[1]) == 1.0 and float(d[0]) == 0.0
    # a constant discounts tensor gives the bits of the number; a duplicate entry those of the list without it
    const = torch.full((B,), c["gamma"], dtype=torch.float32, device=DEV)
    assert torch.equal(head.td_target(xn, r, d, const, ent_coef=ent, noise=noise), head.td_target(xn, r, d, c["gamma"], ent_coef=ent, noise=noise))
    assert torch.equal(head.td_target(xn, r, d, c["gamma"], ent_coef=ent, noise=noise, subset=_sub([N - 1, N - 1][:N])),
                       head.td_target(xn, r, d, c["gamma"], ent_coef=ent, noise=noise, subset=_sub([N - 1])))
    with torch.no_grad():          # against the composition of the other nodes on the same GPU
        a2, lp2 = head.action_log_prob(xn, noise=noise)
        q2 = head.q_values(xn, a2, target=True)
        composed = r + (1 - d) * c["gamma"] * (q2.min(dim=0)[0] - ent * lp2)
    _check_values(name + " target_q against the composition", head.td_target(xn, r, d, c["gamma"], ent_coef=ent, noise=noise), composed.double().cpu().numpy())


def _losses(head, c, target_q):
    """Both losses in both forms with every gradient -> nested dict of CPU tensors."""
    out = {}
    x, a, w = _t(c, "x"), _t(c, "a_replay"), _t(c, "weights")
    for what, kw in (("plain", {}), ("weighted", dict(weights=w, return_td_errors=True)), ("ones", dict(weights=torch.ones_like(w), return_td_errors=True))):
        _clear(head)
        res = head.critic_loss(x, a, target_q, **kw)
        loss, td = res if isinstance(res, tuple) else (res, None)
        assert loss.dim() == 0 and (td is None or (td.shape == target_q.shape and not td.requires_grad))
        (2.0 * loss).backward()          # dloss other than 1
        out["critic_" + what] = dict(loss=loss.detach().cpu(), td=None if td is None else td.cpu(),
                                     grad={n: p.grad.cpu() for n, p in head.named_parameters() if p.grad is not None})
    for reduce in ("min", "mean"):
        _clear(head)
        xg = x.clone().requires_grad_(True)
        loss, logp = head.actor_loss(xg, log_ent_coef=_log_ent(c), noise=_t(c, "noise_pi"), q_reduce=reduce)
        assert loss.dim() == 0 and not logp.requires_grad
        (2.0 * loss).backward()
        grad = {n: p.grad.cpu() for n, p in head.named_parameters() if p.grad is not None}
        grad["x"] = xg.grad.cpu()
        out["actor_" + reduce] = dict(loss=loss.detach().cpu(), logp=logp.cpu(), grad=grad)
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize("name", ALL)
def test_losses_and_their_gradients_against_the_restatement(name):
    """critic_loss plain and weighted with td_abs and every critic gradient, actor_loss with both reductions and every actor gradient and dx,
    each backward with dloss = 2; weights of ones give the bits of no weights; the actor loss leaves the critics alone; two runs give equal bits."""
    c = EC.case(name)
    head = _head(c)
    ent = EC.ent_of(c)
    target_q = head.td_target(_t(c, "x_next"), _t(c, "rewards"), _t(c, "dones"), c["gamma"], ent_coef=ent, noise=_t(c, "noise_next"))
    t64 = target_q.double().cpu().numpy()          # the restatement takes the target the kernels were given
    got, again = _losses(head, c, target_q), _losses(head, c, target_q)
    assert not MG.differing(got, again), "two runs differ in their bits"
    for what, weights in (("plain", None), ("weighted", c["weights"])):
        ref = EC.critic_loss_ref(c, t64, weights)
        g = got["critic_" + what]
        _check_values(f"{name} critic_loss {what}", g["loss"], ref["loss"])
        if weights is not None:
            _check_values(f"{name} td_abs", g["td"], ref["td_abs"])
        assert set(g["grad"]) == set(EC.critic_names(c["arch"], c["n_critics"]))
        _check_grads(f"{name} critic_loss {what}", g["grad"], {k: 2.0 * v for k, v in ref["grad"].items()})
    ones, plain = got["critic_ones"], got["critic_plain"]
    assert torch.equal(ones["loss"], plain["loss"]) and _same(ones["grad"], plain["grad"]), "weights of ones differ from no weights"
    _check_values(name + " td_abs (ones)", ones["td"], EC.critic_loss_ref(c, t64)["td_abs"])
    for reduce in ("min", "mean"):
        ref = EC.actor_loss_ref(c, reduce, ent)
        g = got["actor_" + reduce]
        _check_values(f"{name} actor_loss {reduce}", g["loss"], ref["loss"])
        assert not any(k.startswith("critic") for k in g["grad"]), "actor_loss left a gradient in the critics' parameters"
        _check_grads(f"{name} actor_loss {reduce}", g["grad"], {k: 2.0 * v for k, v in ref["grad"].items()})
    _check_values(name + " log_prob", got["actor_min"]["logp"], EC.reference(name)["log_prob"])


def test_two_critics_anchor_against_sac_head():
    """N = 2, subset None, the min reduction: from the same q, critic_loss (weighted and not), td_abs and actor_loss have SACHead's bits, and so
    have their gradients in q and log_prob.  q, both TD targets, actor_loss, d actions, dx and every parameter gradient through the net walks
    have SACHead's bits too (SACHead's critic entries lift their descriptor to n_critics = 2 and run the ensemble's kernels: this compares the
    lifted call with the direct one), beside the 1e-4 checks against SACHead's values."""
    c = EC.case(EC.ANCHOR)
    ens, twin = _head(c), _head(c, m3l_amd.SACHead)
    x, a, w, logent = _t(c, "x"), _t(c, "a_replay"), _t(c, "weights"), _log_ent(c)
    ent = EC.ent_of(c)
    args = (_t(c, "x_next"), _t(c, "rewards"), _t(c, "dones"))
    with torch.no_grad():
        q = twin.q_values(x, a)
        logp = twin.action_log_prob(x, noise=_t(c, "noise_pi"))[1]
    tq = twin.td_target(*args, c["gamma"], ent_coef=ent, noise=_t(c, "noise_next"))

    def both(fn_ens, fn_twin, leaves):
        res = []
        for fn in (fn_ens, fn_twin):
            ls = [t.clone().requires_grad_(True) for t in leaves]
            out = fn(*ls)
            loss, td = out if isinstance(out, tuple) else (out, None)
            (3.0 * loss).backward()
            res.append([loss.detach(), td] + [t.grad for t in ls])
        torch.cuda.synchronize()
        return res
    for what, (e, t) in (("critic_loss", both(lambda q_: SE.critic_loss_from(q_, tq), lambda q_: SH.critic_loss_from(q_, tq), [q])),
                         ("critic_loss weighted", both(lambda q_: SE.critic_loss_from(q_, tq, w, True), lambda q_: SH.critic_loss_from(q_, tq, w, True), [q])),
                         ("critic_loss td only", both(lambda q_: SE.critic_loss_from(q_, tq, None, True), lambda q_: SH.critic_loss_from(q_, tq, None, True), [q])),
                         ("actor_loss", both(lambda l_, q_: SE.actor_loss_from(l_, q_, log_ent_coef=logent), lambda l_, q_: SH.actor_loss_from(l_, q_, log_ent_coef=logent), [logp, q])),
                         ("actor_loss ent_coef", both(lambda l_, q_: SE.actor_loss_from(l_, q_, ent_coef=ent), lambda l_, q_: SH.actor_loss_from(l_, q_, ent_coef=ent), [logp, q]))):
        for i, (ge, gt) in enumerate(zip(e, t)):
            assert (ge is None) == (gt is None) and (ge is None or torch.equal(ge, gt)), f"{what}: output {i} differs from SACHead's bits"
    # the net walks
    walks = {}
    for label, head, mod in (("ens", ens, SE), ("twin", twin, SH)):
        _clear(head)
        ag = a.clone().requires_grad_(True)
        qh = head.q_values(x, ag)
        qh.backward(torch.ones_like(qh) * w)
        xg = x.clone().requires_grad_(True)
        loss, _ = head.actor_loss(xg, ent_coef=ent, noise=_t(c, "noise_pi"))
        loss.backward()
        torch.cuda.synchronize()
        walks[label] = dict(q=qh.detach(), target_q=head.td_target(*args, c["gamma"], ent_coef=ent, noise=_t(c, "noise_next")),
                            target_rows=head.td_target(*args, _t(c, "discounts"), log_ent_coef=logent, noise=_t(c, "noise_next")),
                            actor_loss=loss.detach(), dactions=ag.grad, dx=xg.grad, **{n: p.grad for n, p in head.named_parameters() if p.grad is not None})
    assert set(walks["ens"]) == set(walks["twin"])
    for k, want in walks["twin"].items():
        got = walks["ens"][k]
        print(f"[anchor] {k}: bits {'equal' if torch.equal(got, want) else 'DIFFER'}")
        assert torch.equal(got, want), f"{k} differs from SACHead's bits"
        if k in ("q", "target_q", "target_rows", "actor_loss"):
            _check_values("anchor " + k, got, want.double().cpu().numpy())
        else:
            _check_grads("anchor " + k, {k: got}, {k: want.double().cpu().numpy()})


def test_ties_go_to_the_lowest_index():
    """Critic 1 a copy of critic 0 (N = 3): under the min reduction critic 0 takes the gradient of every row where the pair is the minimum and
    critic 1 exactly zero there; the target over [1, 0] has the bits of the target over [0]."""
    c = EC.case("a64_n3_b17")
    head = _head(c)
    sd = head.state_dict()
    for k in list(sd):
        if ".qf1." in k:
            sd[k] = sd[k.replace(".qf1.", ".qf0.")].clone()
    ref = EC.reference("a64_n3_b17")["q_pi"]          # critic 2 moves to the pair's median distance, so that it wins about half of the rows
    sd[f"critic.qf2.{2 * len(c['arch'][2])}.bias"] += float(np.median(ref[0] - ref[2]))
    head.load_state_dict(sd)
    x, B = _t(c, "x"), c["x"].shape[0]
    a_pi, logp = head.action_log_prob(x, noise=_t(c, "noise_pi"))
    q = head.q_values(x, a_pi.detach()).detach().requires_grad_(True)
    assert torch.equal(q[0], q[1])
    SE.actor_loss_from(logp.detach(), q, ent_coef=0.2).backward()
    pair = (q[0] <= q[2]).detach()
    assert bool(pair.any()) and bool((~pair).any()), "the case should have rows of both kinds"
    inv = torch.tensor(-1.0 / B, dtype=torch.float32, device=DEV)
    assert torch.equal(q.grad[0], torch.where(pair, inv, torch.zeros_like(inv))) and bool((q.grad[1] == 0).all())
    assert torch.equal(q.grad[2], torch.where(pair, torch.zeros_like(inv), inv))
    args = (_t(c, "x_next"), _t(c, "rewards"), _t(c, "dones"), c["gamma"])
    kw = dict(ent_coef=0.2, noise=_t(c, "noise_next"))
    assert torch.equal(head.td_target(*args, subset=_sub([1, 0]), **kw), head.td_target(*args, subset=_sub([0]), **kw))
    assert torch.equal(head.td_target(*args, subset=_sub([1]), **kw), head.td_target(*args, subset=_sub([0]), **kw))


@pytest.mark.parametrize("name", ["a64_n3_b17", "nohid_n10_b3"])
def test_an_index_outside_the_ensemble_gives_nan_and_touches_nothing(monkeypatch, name):
    """A subset entry of N, -1 or INT_MAX, in any place of the list: every row of target_q is NaN (the host never sees the list), under guarded
    allocations of either fill no byte outside a buffer changes, and a good list right after gives the bits it gave before."""
    c = EC.case(name)
    N = c["n_critics"]
    head = _head(c)
    args = (_t(c, "x_next"), _t(c, "rewards"), _t(c, "dones"), c["gamma"])
    kw = dict(ent_coef=0.2, noise=_t(c, "noise_next"))
    good = head.td_target(*args, subset=_sub([0]), **kw)
    for fill in MG.FILLS:
        with MG.MemGuard(monkeypatch, fill) as g:
            for bad in ([N], [-1], [INT_MAX], [0, N], [-1, 0], [0, INT_MAX, 1][:N]):
                out = head.td_target(*args, subset=_sub(bad), **kw)
                g.check(f"after subset {bad}")
                assert out.shape == good.shape and bool(torch.isnan(out).all()), bad
            assert torch.equal(head.td_target(*args, subset=_sub([0]), **kw), good)
            g.check("after the good list")
            assert g.n_tensors > 0


@pytest.mark.parametrize("name", ["a64_n1_b17", "a64_n10_b33", "mixed_n3_b33"])
def test_polyak_update_moves_all_targets(name):
    c = EC.case(name)
    head = _head(c)
    head.polyak_update(c["tau"])
    torch.cuda.synchronize()
    ref = EC.polyak_ref(c)
    got = {n: p for n, p in head.named_parameters() if n.startswith("critic_target.")}
    assert set(got) == set(ref) and len(ref) == 2 * c["n_critics"] * (len(c["arch"][2]) + 1)
    for k, r in ref.items():
        _check_values(f"{name} {k} after polyak_update", got[k], r)
        assert not torch.equal(got[k].detach().cpu(), torch.from_numpy(c["params"][k])), k
    for n, p in head.named_parameters():
        if not n.startswith("critic_target."):
            assert torch.equal(p.detach().cpu(), torch.from_numpy(c["params"][n])), n


def _contract_step(head, c, g):
    """Every new entry point once: q_values forward and backward, the TD target with a subset and per-row discounts, both losses in both forms
    with their backwards, the Polyak update."""
    _clear(head)
    N = c["n_critics"]
    x, a = _t(c, "x").requires_grad_(True), _t(c, "a_replay")
    target_q = head.td_target(_t(c, "x_next"), _t(c, "rewards"), _t(c, "dones"), _t(c, "discounts"), log_ent_coef=_log_ent(c), noise=_t(c, "noise_next"),
                              subset=_sub([N - 1, 0]))
    full = head.td_target(_t(c, "x_next"), _t(c, "rewards"), _t(c, "dones"), c["gamma"], ent_coef=0.2, noise=_t(c, "noise_next"))
    g.check("after td_target")
    loss, td = head.critic_loss(x, a, target_q, weights=_t(c, "weights"), return_td_errors=True)
    g.check("after critic_loss")
    loss.backward()
    g.check("after critic_loss.backward")
    out = dict(target_q=target_q, full=full, critic_loss=loss.detach(), td=td,
               grad_critic={n: p.grad.clone() for n, p in head.named_parameters() if p.grad is not None})
    plain = head.critic_loss(x, a, full)
    plain.backward()
    g.check("after the unweighted critic_loss")
    out["grad_critic_plain"] = {n: p.grad.clone() for n, p in head.named_parameters() if p.grad is not None}
    _clear(head)
    for reduce in ("min", "mean"):
        al, logp = head.actor_loss(x, ent_coef=0.2, noise=_t(c, "noise_pi"), q_reduce=reduce)
        g.check(f"after actor_loss {reduce}")
        al.backward()
        g.check(f"after actor_loss {reduce} backward")
        out["actor_" + reduce] = dict(loss=al.detach(), logp=logp)
    out["grad_actor"] = {n: p.grad.clone() for n, p in head.named_parameters() if p.grad is not None}
    out["dx"] = x.grad
    head.polyak_update(c["tau"])
    g.check("after polyak_update")
    out["target"] = {n: p.detach().clone() for n, p in head.named_parameters() if n.startswith("critic_target.")}
    return out


@pytest.mark.parametrize("name", CONTRACT)
def test_memory_contract(monkeypatch, name):
    """Every new entry point under guarded, poisoned allocations at ragged-tile shapes: no write outside a buffer, no read of stale workspace,
    padding or outputs, and the bits of the unguarded run."""
    c = EC.case(name)
    params = {k: torch.from_numpy(np.asarray(v)).to(DEV) for k, v in c["params"].items()}
    head = _head(c)

    def work(g):
        with torch.no_grad():
            for n, p in head.named_parameters():
                p.copy_(params[n])          # the Polyak update of the run before is undone
        return _contract_step(head, c, g)
    counts = MG.run_contract(monkeypatch, work)
    # workspaces: the two critic-loss nodes' critics, and per actor loss the actor node's and the critic node's
    assert counts[0] == counts[1] and counts[0][0] == 6, counts


@pytest.mark.parametrize("name", ["mixed_n5_b1", "a64_n10_b33"])
def test_no_grad_calls_take_no_workspace(monkeypatch, name):
    c = EC.case(name)
    head = _head(c)
    x, a, noise = _t(c, "x"), _t(c, "a_replay"), _t(c, "noise_pi")

    def no_grad(g):
        with torch.no_grad():
            out = [head.q_values(x, a), head.q_values(x, a, target=True), head(x, noise=noise)]
        out.append(head.td_target(x, _t(c, "rewards"), _t(c, "dones"), 0.99, ent_coef=0.2, noise=noise, subset=_sub([0])))
        g.check("after the no_grad calls")
        return {"out": out}

    def grad(g):
        q = head.q_values(x, a)
        g.check("after the grad-mode call")
        return {"out": [q.detach()]}
    sized = []
    lib = L.lib()
    real = lib.m3l_sac_ens_ws_bytes
    monkeypatch.setattr(lib, "m3l_sac_ens_ws_bytes", lambda *args: sized.append(1) or real(*args))
    counts = MG.run_contract(monkeypatch, no_grad, need_ws=False)
    assert all(n_ws == 0 for n_ws, _ in counts) and not sized, (counts, len(sized))
    counts = MG.run_contract(monkeypatch, grad)
    assert all(n_ws == 1 for n_ws, _ in counts) and len(sized) == 3
    frozen = _head(c).requires_grad_(False)          # nothing requires a gradient: no workspace in grad mode either
    sized.clear()
    q = frozen.q_values(x.clone().requires_grad_(True), a)          # the features never do, for the critics
    assert not sized and not q.requires_grad
    q = frozen.q_values(x, a.clone().requires_grad_(True))          # the actions do
    assert len(sized) == 1 and q.requires_grad


def test_refusals_that_need_a_device():
    c = EC.case("a64_n3_b17")
    head = _head(c)
    x, a, v = _t(c, "x"), _t(c, "a_replay"), _t(c, "rewards")
    i32 = torch.int32
    for call in (lambda: head(x.cpu()), lambda: head.q_values(x, a.cpu()), lambda: head.q_values(x.cpu(), a), lambda: head.td_target(x, v.cpu(), v, 0.99, ent_coef=0.1),
                 lambda: head.td_target(x, v, v, 0.99, ent_coef=0.1, subset=torch.zeros(2, dtype=i32)), lambda: head.critic_loss(x, a, v.cpu()),
                 lambda: head.critic_loss(x, a, v, weights=v.cpu()), lambda: head.actor_loss(x.cpu(), ent_coef=0.1, q_reduce="mean"),
                 lambda: SE.actor_loss_from(v.cpu(), torch.zeros(3, 17, device=DEV), ent_coef=0.1)):
        with pytest.raises(m3l_amd.M3LError):
            call()
    dev = lambda *s, **k: torch.zeros(*s, device=DEV, **k)      # noqa: E731
    for call in (lambda: head.td_target(x, v, v, 0.99, ent_coef=0.1, subset=dev(2, dtype=torch.int64)), lambda: head.td_target(x, v, v, 0.99, ent_coef=0.1, subset=dev(2)),
                 lambda: head.td_target(x, v, v, 0.99, ent_coef=0.1, subset=dev(4, dtype=i32)), lambda: head.td_target(x, v, v, 0.99, ent_coef=0.1, subset=dev(0, dtype=i32)),
                 lambda: head.td_target(x, v, v, 0.99, ent_coef=0.1, subset=dev(1, 2, dtype=i32)), lambda: head.td_target(x, v, v, 0.99, ent_coef=0.1, subset=dev(4, dtype=i32)[::2]),
                 lambda: head.td_target(x, v, v, 0.99), lambda: head.td_target(x, v[:2], v, 0.99, ent_coef=0.1), lambda: head.q_values(x, a[:2]),
                 lambda: head.critic_loss(x, a, v[:2]), lambda: head.critic_loss(x, a, v, weights=v[:2]), lambda: head.actor_loss(x, ent_coef=0.1, q_reduce="max"),
                 lambda: SE.critic_loss_from(dev(11, 17), v), lambda: SE.actor_loss_from(v[:2], dev(3, 17), ent_coef=0.1)):
        with pytest.raises(ValueError):
            call()
    # the C ABI refuses what the header excludes, with the reason, and writes nothing
    lib = L.lib()
    p = head.params()
    arch = SH._arch(64, p)
    q = torch.full((3, 17), 7.0, device=DEV)
    sub = torch.zeros(2, dtype=i32, device=DEV)
    for change, why in ((dict(n_critics=0), "n_critics"), (dict(n_critics=11), "n_critics"), (dict(features=40), "multiple of 16"), (dict(n_qf=4), "hidden layers"),
                        (dict(B=0), "B >= 1")):
        d = SE._ens_desc(arch, 3, actor=p.actor_flat(), critic=p.critic_flat())
        B = change.pop("B", 17)
        for k, val in change.items():
            setattr(d, k, val)
        assert lib.m3l_sac_ens_critic_fwd(C.byref(d), B, L.ptr(x), L.ptr(a), None, L.ptr(q), None) != 0 and why in L.last_error(), L.last_error()
        assert lib.m3l_sac_ens_td_target(C.byref(d), B, L.ptr(x), None, L.ptr(v), L.ptr(v), None, 0.99, 0.1, None, None, 0, L.ptr(q), None) != 0
    d = SE._ens_desc(arch, 3, actor=p.actor_flat(), critic=p.critic_flat())
    for n_subset in (0, 4, -1):
        assert lib.m3l_sac_ens_td_target(C.byref(d), 17, L.ptr(x), None, L.ptr(v), L.ptr(v), None, 0.99, 0.1, None, L.ptr(sub), n_subset, L.ptr(q), None) != 0
        assert "n_subset" in L.last_error()
    assert lib.m3l_sac_ens_critic_fwd(C.byref(SE._ens_desc(arch, 3, actor=p.actor_flat())), 17, L.ptr(x), L.ptr(a), None, L.ptr(q), None) != 0 and "null" in L.last_error()
    assert lib.m3l_sac_ens_critic_loss_fwd(L.ptr(q), L.ptr(v), None, 11, 17, L.ptr(q), L.ptr(q), None, None) != 0
    assert lib.m3l_sac_ens_actor_loss_fwd(L.ptr(v), L.ptr(q), 3, 17, 2, 0.1, None, L.ptr(q), L.ptr(q), None) != 0 and "reduce" in L.last_error()
    assert lib.m3l_sac_ens_loss_bwd(L.ptr(v), L.ptr(q), 0, L.ptr(q), None) != 0
    torch.cuda.synchronize()
    assert bool((q == 7.0).all())
