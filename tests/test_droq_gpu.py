"""GPU checks of the SAC DroQ critics (m3l_sac_droq_*, m3l_amd.SACEnsembleHead(critic_layer_norm=True, critic_dropout=p), m3l_amd/sac_ensemble.py).

Yardstick: the float64 restatement of tests/droq_cases.py, whose masks are test_dropout_cpu.dropout_mask's (pinned by known answers) and whose
LayerNorm-off form test_droq_cpu.py pins to sac_ens_cases.  Every input satisfies the conditions test_droq_cpu.py asserts: every post-LayerNorm
value in front of a ReLU at least GATE_MARGIN from 0 in every evaluation made here, the two smallest values at least TIE_MARGIN apart wherever a
minimum is taken, so the gates and the chosen critic are the same in float32 and float64.  Every call that drops gets an injected dropout_seed.
Bounds, the existing head's (test_sac_head_gpu.py): values within 1e-4 of max(1, |ref|), every gradient tensor within 1e-4 of its largest
float64 entry.  Measured on an MI355X (EXPERIMENTS.md 5.32): values within 1.6e-6, gradients within 2.4e-6."""
import numpy as np
import pytest
import torch

import droq_cases as DC
import m3l_amd
import memguard as MG
import sac_ens_cases as EC
from m3l_amd import _lib as L
from m3l_amd import sac_ensemble as SE
from test_sac_head_gpu import _check_grads, _check_values, _clear

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ALL = list(DC.CASES)
CONTRACT = ["mixed_n3_b33_p10", "amax_n3_b3_p10", "w512_n1_b17_p10"]
SQ, ST = DC.SEED_Q, DC.SEED_T


def _head(c):
    Fd, pi, qf, A = c["arch"]
    head = m3l_amd.SACEnsembleHead(Fd, A, net_arch=dict(pi=list(pi), qf=list(qf)), n_critics=c["n_critics"], critic_layer_norm=True,
                                   critic_dropout=c["dropout_p"])
    assert list(head.state_dict().keys()) == DC.param_names(c["arch"], c["n_critics"])
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


def _drops(c):
    return c["dropout_p"] > 0 and len(c["arch"][2]) > 0


@pytest.mark.parametrize("name", ALL)
def test_q_values_forward_and_backward_against_the_restatement(name):
    """All N critics at (x, a_replay) under the injected seed with a random output gradient: q (N, B), d actions and every gradient (W, b, gamma,
    beta of every critic and layer); the features take none; two runs with one seed give equal bits; the d-actions-only mode and the no_grad
    call give the same bits; target=True reads critic_target's tensors, LayerNorm ones included."""
    c = DC.case(name)
    N, B = c["n_critics"], c["x"].shape[0]
    dq = torch.randn(N, B, generator=torch.Generator().manual_seed(11))
    ref = DC.q_ref(c, c["a_replay"], dq.numpy())
    head = _head(c)
    runs = []
    for mode in ("full", "full", "actions_only"):
        _clear(head)
        x = _t(c, "x").requires_grad_(True)
        a = _t(c, "a_replay").requires_grad_(True)
        q = head.q_values(x, a, dropout_seed=SQ) if mode == "full" else SE.q_values(head.params(), x, a, param_grads=False, dropout_seed=SQ)
        assert q.shape == (N, B) and q.dtype == torch.float32 and q.requires_grad
        q.backward(dq.to(DEV))
        torch.cuda.synchronize()
        assert x.grad is None, "the features enter the critics detached"
        grads = {n: p.grad.cpu() for n, p in head.named_parameters() if p.grad is not None}
        grads["actions"] = a.grad.cpu()
        runs.append((q.detach().cpu(), grads))
    assert torch.equal(runs[0][0], runs[1][0]) and _same(runs[0][1], runs[1][1]), "two runs with one seed differ in their bits"
    assert set(runs[2][1]) == {"actions"} and torch.equal(runs[2][1]["actions"], runs[0][1]["actions"]) and torch.equal(runs[2][0], runs[0][0])
    assert set(runs[0][1]) == set(DC.critic_names(c["arch"], N)) | {"actions"}
    _check_values(name + " q", runs[0][0], ref["q"])
    _check_grads(name, runs[0][1], ref["grad"])
    if _drops(c):
        assert head.last_dropout_seeds["q_values"] == SQ
    with torch.no_grad():
        quiet = head.q_values(_t(c, "x"), _t(c, "a_replay"), dropout_seed=SQ)
        qt = head.q_values(_t(c, "x"), _t(c, "a_replay"), target=True, dropout_seed=SQ)
    assert torch.equal(quiet.cpu(), runs[0][0]) and not quiet.requires_grad
    _check_values(name + " target q", qt, DC.q_ref(c, c["a_replay"], dq.numpy(), prefix="critic_target")["q"])


@pytest.mark.parametrize("name", ALL)
def test_seeds_and_eval_mode(name):
    """Two seeds give different q where something drops (p > 0 and a hidden layer) and equal bits where nothing does; a call without a seed
    draws one from torch's CPU generator and keeps it; head.critic.eval() makes q independent of the seed and equal, with its gradients, to the
    restatement with all-ones masks and scale 1."""
    c = DC.case(name)
    N, B = c["n_critics"], c["x"].shape[0]
    head = _head(c)
    x, a = _t(c, "x"), _t(c, "a_replay")
    with torch.no_grad():
        q1, q2 = head.q_values(x, a, dropout_seed=SQ), head.q_values(x, a, dropout_seed=ST)
        assert torch.equal(q1, q2) != _drops(c), "whether the seed matters"
        torch.manual_seed(21)
        drawn = head.q_values(x, a)
        if _drops(c):
            seed = head.last_dropout_seeds["q_values"]
            torch.manual_seed(21)
            assert seed not in (SQ, ST) and head.q_values(x, a).equal(drawn) and head.q_values(x, a, dropout_seed=seed).equal(drawn)
            assert not torch.equal(drawn, q1)
        else:
            assert torch.equal(drawn, q1)
    head.critic.eval()
    dq = torch.randn(N, B, generator=torch.Generator().manual_seed(12))
    ref = DC.q_ref(c, c["a_replay"], dq.numpy(), seed=None)
    ag = a.clone().requires_grad_(True)
    q = head.q_values(x, ag, dropout_seed=SQ)
    q.backward(dq.to(DEV))
    with torch.no_grad():
        assert torch.equal(head.q_values(x, a, dropout_seed=ST), q.detach()) and torch.equal(head.q_values(x, a), q.detach())
    grads = {n: p.grad for n, p in head.named_parameters() if p.grad is not None}
    grads["actions"] = ag.grad
    _check_values(name + " q (eval)", q, ref["q"])
    _check_grads(name + " (eval)", grads, ref["grad"])
    if not _drops(c):
        assert torch.equal(q.detach(), q1)


@pytest.mark.parametrize("name", ALL)
def test_td_target_for_every_subset_against_the_restatement(name):
    """One launch per call: every subset of the case with critic_target in train mode (the DroQ paper's rule: the target drops, each critic under
    its own index's masks) and in eval mode (SB3's rule); gamma as a number and as one discount per row; against the restatement and against
    the composition action_log_prob -> q_values(target=True) with the same seed on the GPU; two calls with one seed give equal bits."""
    c, ref = DC.case(name), DC.reference(name)
    N, B = c["n_critics"], c["x"].shape[0]
    head = _head(c)
    xn, r, d, noise, disc = _t(c, "x_next"), _t(c, "rewards"), _t(c, "dones"), _t(c, "noise_next"), _t(c, "discounts")
    ent = EC.ent_of(c)
    for train in (True, False):
        head.critic_target.train(train)
        with torch.no_grad():
            a2, lp2 = head.action_log_prob(xn, noise=noise)
            q2 = head.q_values(xn, a2, target=True, dropout_seed=ST)
        for sub in EC.subsets(N):
            s = _sub(sub)
            by_float = head.td_target(xn, r, d, c["gamma"], ent_coef=ent, noise=noise, subset=s, dropout_seed=ST)
            by_ptr = head.td_target(xn, r, d, c["gamma"], log_ent_coef=_log_ent(c), noise=noise, subset=s, dropout_seed=ST)
            rows = head.td_target(xn, r, d, disc.reshape(B, 1), ent_coef=ent, noise=noise, subset=s, dropout_seed=ST)
            again = head.td_target(xn, r, d, c["gamma"], ent_coef=ent, noise=noise, subset=s, dropout_seed=ST)
            assert by_float.shape == (B,) and not by_float.requires_grad and torch.equal(by_float, again)
            what = f"{name} target_q {sub} ({'train' if train else 'eval'})"
            _check_values(what + " (float)", by_float, DC.target_ref(c, ref, sub, c["gamma"], ent, train))
            _check_values(what + " (pointer)", by_ptr, DC.target_ref(c, ref, sub, c["gamma"], ent, train))
            _check_values(what + " (per-row discounts)", rows, DC.target_ref(c, ref, sub, c["discounts"], ent, train))
            composed = r + (1 - d) * c["gamma"] * ((q2 if sub is None else q2[sub]).min(dim=0)[0] - ent * lp2)
            _check_values(what + " against the composition", by_float, composed.double().cpu().numpy())
            other = head.td_target(xn, r, d, c["gamma"], ent_coef=ent, noise=noise, subset=s, dropout_seed=SQ)
            live = (d == 0)
            assert torch.equal(other, by_float) != (train and _drops(c) and bool(live.any())), "whether the seed matters to the target"
            if B > 1:
                assert torch.equal(by_float[1], r[1]) and float(d[1]) == 1.0 and float(d[0]) == 0.0
        if train and _drops(c):
            assert head.last_dropout_seeds["td_target"] == SQ


def _losses(head, c, target_q):
    """Both losses in both forms with every gradient, under the injected seed -> nested dict of CPU tensors."""
    out = {}
    x, a, w = _t(c, "x"), _t(c, "a_replay"), _t(c, "weights")
    for what, kw in (("plain", {}), ("weighted", dict(weights=w, return_td_errors=True)), ("ones", dict(weights=torch.ones_like(w), return_td_errors=True))):
        _clear(head)
        res = head.critic_loss(x, a, target_q, dropout_seed=SQ, **kw)
        loss, td = res if isinstance(res, tuple) else (res, None)
        assert loss.dim() == 0 and (td is None or (td.shape == target_q.shape and not td.requires_grad))
        (2.0 * loss).backward()          # dloss other than 1
        out["critic_" + what] = dict(loss=loss.detach().cpu(), td=None if td is None else td.cpu(),
                                     grad={n: p.grad.cpu() for n, p in head.named_parameters() if p.grad is not None})
    for reduce in ("min", "mean"):
        _clear(head)
        xg = x.clone().requires_grad_(True)
        loss, logp = head.actor_loss(xg, log_ent_coef=_log_ent(c), noise=_t(c, "noise_pi"), q_reduce=reduce, dropout_seed=SQ)
        assert loss.dim() == 0 and not logp.requires_grad
        (2.0 * loss).backward()
        grad = {n: p.grad.cpu() for n, p in head.named_parameters() if p.grad is not None}
        grad["x"] = xg.grad.cpu()
        out["actor_" + reduce] = dict(loss=loss.detach().cpu(), logp=logp.cpu(), grad=grad)
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize("name", ALL)
def test_losses_and_their_gradients_against_the_restatement(name):
    """critic_loss plain and weighted with td_abs and every critic gradient (LayerNorm ones included), actor_loss with both reductions and
    every actor gradient and dx, each backward with dloss = 2; weights of ones give the bits of no weights; the actor loss leaves the critics
    alone; two runs give equal bits."""
    c = DC.case(name)
    head = _head(c)
    ent = EC.ent_of(c)
    target_q = head.td_target(_t(c, "x_next"), _t(c, "rewards"), _t(c, "dones"), c["gamma"], ent_coef=ent, noise=_t(c, "noise_next"), dropout_seed=ST)
    t64 = target_q.double().cpu().numpy()          # the restatement takes the target the kernels were given
    got, again = _losses(head, c, target_q), _losses(head, c, target_q)
    assert not MG.differing(got, again), "two runs differ in their bits"
    for what, weights in (("plain", None), ("weighted", c["weights"])):
        ref = DC.critic_loss_ref(c, t64, weights)
        g = got["critic_" + what]
        _check_values(f"{name} critic_loss {what}", g["loss"], ref["loss"])
        if weights is not None:
            _check_values(f"{name} td_abs", g["td"], ref["td_abs"])
        assert set(g["grad"]) == set(DC.critic_names(c["arch"], c["n_critics"]))
        _check_grads(f"{name} critic_loss {what}", g["grad"], {k: 2.0 * v for k, v in ref["grad"].items()})
    ones, plain = got["critic_ones"], got["critic_plain"]
    assert torch.equal(ones["loss"], plain["loss"]) and _same(ones["grad"], plain["grad"]), "weights of ones differ from no weights"
    for reduce in ("min", "mean"):
        ref = DC.actor_loss_ref(c, reduce, ent)
        g = got["actor_" + reduce]
        _check_values(f"{name} actor_loss {reduce}", g["loss"], ref["loss"])
        assert not any(k.startswith("critic") for k in g["grad"]), "actor_loss left a gradient in the critics' parameters"
        _check_grads(f"{name} actor_loss {reduce}", g["grad"], {k: 2.0 * v for k, v in ref["grad"].items()})
    _check_values(name + " log_prob", got["actor_min"]["logp"], DC.reference(name)["log_prob"])


@pytest.mark.parametrize("name", ["mixed_n3_b33_p10", "a64_n2_b17_p01"])
def test_polyak_update_moves_all_targets(name):
    """Every tensor of the target critics, gamma and beta included, and nothing else."""
    c = DC.case(name)
    head = _head(c)
    head.polyak_update(c["tau"])
    torch.cuda.synchronize()
    ref = EC.polyak_ref(c)
    got = {n: p for n, p in head.named_parameters() if n.startswith("critic_target.")}
    assert set(got) == set(ref) == set(DC.critic_names(c["arch"], c["n_critics"], "critic_target"))
    assert len(ref) == c["n_critics"] * (4 * len(c["arch"][2]) + 2) and any(".2.weight" in k for k in ref)
    for k, r in ref.items():
        _check_values(f"{name} {k} after polyak_update", got[k], r)
        assert not torch.equal(got[k].detach().cpu(), torch.from_numpy(c["params"][k])), k
    for n, p in head.named_parameters():
        if not n.startswith("critic_target."):
            assert torch.equal(p.detach().cpu(), torch.from_numpy(c["params"][n])), n


def test_default_head_makes_no_droq_call(monkeypatch):
    """SACEnsembleHead with both arguments at their defaults: every m3l_sac_droq_* symbol may raise and a whole step still runs, and at N = 2 its
    q, target, losses and gradients have SACHead's bits."""
    lib = L.lib()

    def boom(*a):
        raise AssertionError("a head without LayerNorm called a DroQ entry")
    for s in L.EXPORTS:
        if s.startswith("m3l_sac_droq_"):
            monkeypatch.setattr(lib, s, boom)
    c = EC.case(EC.ANCHOR)
    Fd, pi, qf, A = c["arch"]
    sd = {k: torch.from_numpy(np.asarray(v)) for k, v in c["params"].items()}
    out = {}
    for label, head in (("ens", m3l_amd.SACEnsembleHead(Fd, A, net_arch=dict(pi=list(pi), qf=list(qf)), n_critics=2)),
                        ("twin", m3l_amd.SACHead(Fd, A, net_arch=dict(pi=list(pi), qf=list(qf))))):
        head.load_state_dict(sd, strict=True)
        head.to(DEV)
        x, a = _t(c, "x"), _t(c, "a_replay").requires_grad_(True)
        tq = head.td_target(_t(c, "x_next"), _t(c, "rewards"), _t(c, "dones"), c["gamma"], ent_coef=0.2, noise=_t(c, "noise_next"))
        q = head.q_values(x, a)
        q.backward(torch.ones_like(q))
        res = dict(q=q.detach(), target_q=tq, dactions=a.grad, **{"q " + n: p.grad for n, p in head.named_parameters() if p.grad is not None})
        _clear(head)
        cl = head.critic_loss(x, a.detach(), tq)
        cl.backward()
        res.update(critic_loss=cl.detach(), **{"cl " + n: p.grad for n, p in head.named_parameters() if p.grad is not None})
        _clear(head)
        al, _ = head.actor_loss(x, ent_coef=0.2, noise=_t(c, "noise_pi"))
        al.backward()
        res.update(actor_loss=al.detach(), **{"al " + n: p.grad for n, p in head.named_parameters() if p.grad is not None})
        torch.cuda.synchronize()
        out[label] = res
    assert not MG.differing(out["ens"], out["twin"]), MG.differing(out["ens"], out["twin"])
    with pytest.raises(AssertionError, match="DroQ entry"):          # the patch bites: a DroQ head does go there
        with torch.no_grad():
            _head(DC.case(DC.ANCHOR)).q_values(_t(DC.case(DC.ANCHOR), "x"), _t(DC.case(DC.ANCHOR), "a_replay"), dropout_seed=SQ)


def _contract_step(head, c, g):
    """The three new entry points: q_values forward and backward, the TD target with a subset and per-row discounts in train and in eval mode,
    and through both losses with their backwards; then the Polyak update."""
    _clear(head)
    N = c["n_critics"]
    x, a = _t(c, "x").requires_grad_(True), _t(c, "a_replay")
    head.critic_target.train()
    target_q = head.td_target(_t(c, "x_next"), _t(c, "rewards"), _t(c, "dones"), _t(c, "discounts"), log_ent_coef=_log_ent(c), noise=_t(c, "noise_next"),
                              subset=_sub([N - 1, 0][:N]), dropout_seed=ST)
    head.critic_target.eval()
    full = head.td_target(_t(c, "x_next"), _t(c, "rewards"), _t(c, "dones"), c["gamma"], ent_coef=0.2, noise=_t(c, "noise_next"), dropout_seed=ST)
    head.critic_target.train()
    g.check("after td_target")
    loss, td = head.critic_loss(x, a, target_q, weights=_t(c, "weights"), return_td_errors=True, dropout_seed=SQ)
    g.check("after critic_loss")
    loss.backward()
    g.check("after critic_loss.backward")
    out = dict(target_q=target_q, full=full, critic_loss=loss.detach(), td=td,
               grad_critic={n: p.grad.clone() for n, p in head.named_parameters() if p.grad is not None})
    head.critic.eval()
    plain = head.critic_loss(x, a, full)
    plain.backward()
    head.critic.train()
    g.check("after the critic_loss in eval mode")
    out["grad_critic_eval"] = {n: p.grad.clone() for n, p in head.named_parameters() if p.grad is not None}
    _clear(head)
    for reduce in ("min", "mean"):
        al, logp = head.actor_loss(x, ent_coef=0.2, noise=_t(c, "noise_pi"), q_reduce=reduce, dropout_seed=SQ)
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
    """The new entry points under guarded, poisoned allocations of exact size at ragged-tile shapes (three LayerNorm sites with a width that is
    no multiple of 64; no site at all; the 512-wide layer): no write outside a buffer, no read of stale workspace, padding or outputs, and the
    bits of the unguarded run."""
    c = DC.case(name)
    params = {k: torch.from_numpy(np.asarray(v)).to(DEV) for k, v in c["params"].items()}
    head = _head(c)
    sized = []
    lib = L.lib()
    real = lib.m3l_sac_droq_ws_bytes
    monkeypatch.setattr(lib, "m3l_sac_droq_ws_bytes", lambda *args: sized.append(1) or real(*args))

    def work(g):
        with torch.no_grad():
            for n, p in head.named_parameters():
                p.copy_(params[n])          # the Polyak update of the run before is undone
        return _contract_step(head, c, g)
    counts = MG.run_contract(monkeypatch, work)
    # workspaces: the two critic-loss nodes' critics, and per actor loss the actor node's and the critic node's; the critics' are all DroQ-sized
    assert counts[0] == counts[1] and counts[0][0] == 6 and len(sized) == 3 * 4, (counts, len(sized))
