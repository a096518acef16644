"""GPU checks of the TQC head (m3l_tqc_*, m3l_amd.TQCHead, m3l_amd/tqc.py).

Yardstick: the float64 restatement of tests/tqc_cases.py, which test_tqc_cpu.py pins to a loop-written second version and a hand-computed
example.  Bounds, the SAC head tests': every tensor within 1e-4 of the float64 tensor's largest absolute entry, every scalar within
1e-4 * max(1, |value|).  The loss and its gradient are continuous in every input, so nothing is asked of delta; the ReLU gates of the nets are
settled by sac_ens_cases at every point where a gradient is taken.  Measured on an MI355X (EXPERIMENTS.md 5.33): tensors within 2.2e-6, gradients
within 2.7e-6 of their largest entry, scalars within 1.7e-7."""
import ctypes as C

import numpy as np
import pytest
import torch

import m3l_amd
import memguard as MG
import sac_ens_cases as EC
import tqc_cases as TC
from m3l_amd import _lib as L
from m3l_amd import tqc as TQ

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ALL = list(TC.CASES)
TOL = 1e-4
CONTRACT = ["f16_a1_q32_n3q5d4_b1", "f16_a7_q32_n10q25d2_b17", TC.STEP]          # B = 1; the largest pool; the whole step's shape


def _head(c, drop=None, params=None):
    Fd, pi, qf, A = c["arch"]
    head = m3l_amd.TQCHead(Fd, A, net_arch=dict(pi=list(pi), qf=list(qf)), n_critics=c["n_critics"], n_quantiles=c["n_quantiles"],
                           top_quantiles_to_drop_per_net=c["drop"] if drop is None else drop)
    head.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in (params or c["params"]).items()}, strict=True)
    return head.to(DEV)


def _t(c, k):
    return torch.from_numpy(c[k]).to(DEV)


def _log_ent(c):
    return torch.tensor([c["log_ent_coef"]], dtype=torch.float32, device=DEV)


def _clear(head):
    for p in head.parameters():
        p.grad = None


def _check(what, got, ref):
    """A tensor within TOL of the float64 tensor's largest absolute entry; a scalar within TOL * max(1, |value|)."""
    got = got.detach().double().cpu().numpy() if isinstance(got, torch.Tensor) else np.asarray(got, dtype=np.float64)
    ref = np.asarray(ref, dtype=np.float64)
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    scale = max(1.0, abs(float(ref))) if ref.ndim == 0 else float(np.abs(ref).max())
    err = float(np.abs(got - ref).max()) / scale if scale > 0 else (0.0 if not np.any(got) else float("inf"))
    print(f"[{what}] err {err:.2e} of {'max(1, |value|)' if ref.ndim == 0 else 'the largest entry'} (bound {TOL:.0e})")
    assert err <= TOL, (what, err, scale)


def _check_grads(what, got, ref):
    assert set(got) == set(ref), set(got) ^ set(ref)
    for k, r in ref.items():
        _check(f"{what} grad {k}", got[k], r)


def _same(a, b):
    return set(a) == set(b) and all(torch.equal(a[k], b[k]) for k in a)


@pytest.mark.parametrize("name", ALL)
def test_quantiles_forward_and_backward_against_the_restatement(name):
    """All N critics at (x, a_replay) with a random output gradient: z (N, B, nq) contiguous, d actions (the chain over the critics) and every
    critic gradient (the grouped launches, the [nq, w] head among them); the features take none; two runs give equal bits; the d-actions-only
    mode and the no_grad call give the same bits; target=True reads critic_target."""
    c = TC.case(name)
    N, B, nq = c["n_critics"], c["x"].shape[0], c["n_quantiles"]
    dz = torch.randn(N, B, nq, generator=torch.Generator().manual_seed(11))
    ref = TC.z_ref(c, c["a_replay"], dz.numpy())
    head = _head(c)
    runs = []
    for mode in ("full", "full", "actions_only"):
        _clear(head)
        x = _t(c, "x").requires_grad_(True)
        a = _t(c, "a_replay").requires_grad_(True)
        z = head.quantiles(x, a) if mode == "full" else TQ.quantiles(head.params(), x, a, param_grads=False)
        assert z.shape == (N, B, nq) and z.dtype == torch.float32 and z.requires_grad and z.is_contiguous()
        z.backward(dz.to(DEV))
        torch.cuda.synchronize()
        assert x.grad is None, "the features enter the critics detached"
        grads = {n: p.grad.cpu() for n, p in head.named_parameters() if p.grad is not None}
        grads["actions"] = a.grad.cpu()
        runs.append((z.detach().cpu(), grads))
    assert torch.equal(runs[0][0], runs[1][0]) and _same(runs[0][1], runs[1][1]), "two runs differ in their bits"
    assert set(runs[2][1]) == {"actions"} and torch.equal(runs[2][1]["actions"], runs[0][1]["actions"]) and torch.equal(runs[2][0], runs[0][0])
    _check(name + " z", runs[0][0], ref["z"])
    _check_grads(name, runs[0][1], ref["grad"])
    with torch.no_grad():
        quiet = head.quantiles(_t(c, "x"), _t(c, "a_replay"))
        zt = head.quantiles(_t(c, "x"), _t(c, "a_replay"), target=True)
    assert torch.equal(quiet.cpu(), runs[0][0]) and not quiet.requires_grad
    _check(name + " target z", zt, TC.z_ref(c, c["a_replay"], dz.numpy(), prefix="critic_target")["z"])


@pytest.mark.parametrize("name", ALL)
def test_td_target_against_the_restatement(name):
    """One launch per call: gamma as a number and as one discount per row, the entropy coefficient as a number and as a pointer to its
    logarithm, the actor noisy and deterministic (a draw of zeros); a done row is its reward in every column; the kept quantiles ascend; two
    calls give equal bits; and the composition of the other nodes with torch.sort on the same GPU agrees."""
    c = TC.case(name)
    B, K = c["x"].shape[0], c["K"]
    head = _head(c)
    xn, r, d, noise, disc = _t(c, "x_next"), _t(c, "rewards"), _t(c, "dones"), _t(c, "noise_next"), _t(c, "discounts")
    ent = TC.ent_of(c)
    by_float = head.td_target(xn, r, d, c["gamma"], ent_coef=ent, noise=noise)
    by_ptr = head.td_target(xn, r, d, c["gamma"], log_ent_coef=_log_ent(c), noise=noise)
    rows = head.td_target(xn, r, d, disc.reshape(B, 1), ent_coef=ent, noise=noise)
    again = head.td_target(xn, r, d, c["gamma"], ent_coef=ent, noise=noise)
    quiet = head.td_target(xn, r, d, c["gamma"], ent_coef=ent, noise=torch.zeros_like(noise))
    assert by_float.shape == (B, K) and by_float.dtype == torch.float32 and not by_float.requires_grad and torch.equal(by_float, again)
    _check(f"{name} target (float)", by_float, TC.target_ref(c, c["gamma"], ent))
    _check(f"{name} target (pointer)", by_ptr, TC.target_ref(c, c["gamma"], ent))
    _check(f"{name} target (per-row discounts)", rows, TC.target_ref(c, c["discounts"], ent))
    _check(f"{name} target (deterministic actor)", quiet, TC.target_ref(c, c["gamma"], ent, noise_next=np.zeros_like(c["noise_next"])))
    assert bool((by_float[d == 0].diff(dim=1) >= 0).all()), "the kept quantiles of a row ascend"
    if B > 1:
        assert torch.equal(by_float[1], r[1].expand(K)) and float(d[1]) == 1.0 and float(d[0]) == 0.0
    const = torch.full((B,), c["gamma"], dtype=torch.float32, device=DEV)
    assert torch.equal(head.td_target(xn, r, d, const, ent_coef=ent, noise=noise), by_float), "a constant discounts tensor differs from the number"
    with torch.no_grad():          # against the composition of the other nodes on the same GPU
        a2, lp2 = head.action_log_prob(xn, noise=noise)
        z2 = head.quantiles(xn, a2, target=True)
        pooled = torch.sort(z2.permute(1, 0, 2).reshape(B, -1))[0][:, :K]
        composed = r.reshape(-1, 1) + (1 - d.reshape(-1, 1)) * c["gamma"] * (pooled - ent * lp2.reshape(-1, 1))
    _check(name + " target against the composition", by_float, composed.double().cpu().numpy())


def _losses(head, c, target):
    """Both losses with every gradient -> nested dict of CPU tensors."""
    out = {}
    x, a, w = _t(c, "x"), _t(c, "a_replay"), _t(c, "weights")
    for what, kw in (("plain", {}), ("weighted", dict(weights=w.reshape(-1, 1), return_td_errors=True)),
                     ("ones", dict(weights=torch.ones_like(w), return_td_errors=True))):
        _clear(head)
        res = head.critic_loss(x, a, target, **kw)
        loss, td = res if isinstance(res, tuple) else (res, None)
        assert loss.dim() == 0 and (td is None or (td.shape == (x.shape[0],) and not td.requires_grad))
        (2.0 * loss).backward()          # dloss other than 1
        out["critic_" + what] = dict(loss=loss.detach().cpu(), td=None if td is None else td.cpu(),
                                     grad={n: p.grad.cpu() for n, p in head.named_parameters() if p.grad is not None})
    _clear(head)
    xg = x.clone().requires_grad_(True)
    loss, logp = head.actor_loss(xg, log_ent_coef=_log_ent(c), noise=_t(c, "noise_pi"))
    assert loss.dim() == 0 and not logp.requires_grad
    (2.0 * loss).backward()
    grad = {n: p.grad.cpu() for n, p in head.named_parameters() if p.grad is not None}
    grad["x"] = xg.grad.cpu()
    out["actor"] = dict(loss=loss.detach().cpu(), logp=logp.cpu(), grad=grad)
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize("name", ALL)
def test_losses_and_their_gradients_against_the_restatement(name):
    """critic_loss plain and weighted with td errors and every critic gradient, actor_loss with every actor gradient and dx, each backward with
    dloss = 2; weights of ones give the bits of no weights; the actor loss leaves the critics alone; two runs give equal bits."""
    c = TC.case(name)
    head = _head(c)
    ent = TC.ent_of(c)
    target = head.td_target(_t(c, "x_next"), _t(c, "rewards"), _t(c, "dones"), c["gamma"], ent_coef=ent, noise=_t(c, "noise_next"))
    t64 = target.double().cpu().numpy()          # the restatement takes the target the kernels were given
    got, again = _losses(head, c, target), _losses(head, c, target)
    assert not MG.differing(got, again), "two runs differ in their bits"
    for what, weights in (("plain", None), ("weighted", c["weights"])):
        ref = TC.critic_loss_ref(c, t64, weights)
        g = got["critic_" + what]
        _check(f"{name} critic_loss {what}", g["loss"], ref["loss"])
        if weights is not None:
            _check(f"{name} td", g["td"], ref["td_abs"])
        assert set(g["grad"]) == set(TC.critic_names(c["arch"], c["n_critics"]))
        _check_grads(f"{name} critic_loss {what}", g["grad"], {k: 2.0 * v for k, v in ref["grad"].items()})
    ones, plain = got["critic_ones"], got["critic_plain"]
    assert torch.equal(ones["loss"], plain["loss"]) and _same(ones["grad"], plain["grad"]), "weights of ones differ from no weights"
    _check(name + " td (ones)", ones["td"], TC.critic_loss_ref(c, t64)["td_abs"])
    ref = TC.actor_loss_ref(c, ent)
    g = got["actor"]
    _check(f"{name} actor_loss", g["loss"], ref["loss"])
    assert not any(k.startswith("critic") for k in g["grad"]), "actor_loss left a gradient in the critics' parameters"
    _check_grads(f"{name} actor_loss", g["grad"], {k: 2.0 * v for k, v in ref["grad"].items()})
    _check(name + " log_prob", g["logp"], ref["log_prob"])
    # the coefficients by themselves: d loss / d z from a leaf z
    z = head.quantiles(_t(c, "x"), _t(c, "a_replay")).detach().requires_grad_(True)
    TQ.critic_loss_from(z, target, _t(c, "weights")).backward()
    z64 = TC.critic_loss_ref(c, t64, c["weights"])
    _check(name + " d loss / d z", z.grad, z64["coef"])


@pytest.mark.parametrize("drop", [0, 1, 24])
def test_ties_in_the_pool(drop):
    """critic_target.qf1 loaded with qf0's weights: every pooled value occurs twice.  Only values are output, so the restatement's torch.sort
    and the rank count agree whatever the order of equal entries; d = 0 keeps all, 1 cuts a pair, nq - 1 keeps one pair."""
    base = TC.case("f32_a7_q32_n2q25d2_b17")
    params = dict(base["params"])
    for k in list(params):
        if k.startswith("critic_target.qf1."):
            params[k] = params[k.replace(".qf1.", ".qf0.")].copy()
    c = dict(base, params=params, drop=drop, K=TC.kept(2, 25, drop))
    head = _head(c)
    ent = TC.ent_of(c)
    got = head.td_target(_t(c, "x_next"), _t(c, "rewards"), _t(c, "dones"), _t(c, "discounts"), ent_coef=ent, noise=_t(c, "noise_next"))
    assert got.shape == (17, 2 * (25 - drop))
    assert torch.equal(got[:, 0::2], got[:, 1::2]), "every kept value occurs twice"
    _check(f"ties d={drop} target", got, TC.target_ref(c, c["discounts"], ent))


def _step(head, c):
    """td_target -> critic_loss.backward() -> actor_loss.backward() -> polyak_update, everything kept."""
    _clear(head)
    x = _t(c, "x").requires_grad_(True)
    target = head.td_target(_t(c, "x_next"), _t(c, "rewards"), _t(c, "dones"), _t(c, "discounts"), log_ent_coef=_log_ent(c), noise=_t(c, "noise_next"))
    closs, td = head.critic_loss(x, _t(c, "a_replay"), target, weights=_t(c, "weights"), return_td_errors=True)
    closs.backward()
    out = dict(target=target, critic_loss=closs.detach(), td=td, grad_critic={n: p.grad.clone() for n, p in head.named_parameters() if p.grad is not None})
    _clear(head)
    aloss, logp = head.actor_loss(x, log_ent_coef=_log_ent(c), noise=_t(c, "noise_pi"))
    aloss.backward()
    out.update(actor_loss=aloss.detach(), logp=logp, grad_actor={n: p.grad.clone() for n, p in head.named_parameters() if p.grad is not None}, dx=x.grad)
    head.polyak_update(c["tau"])
    out["moved"] = {n: p.detach().clone() for n, p in head.named_parameters() if n.startswith("critic_target.")}
    torch.cuda.synchronize()
    return out


def test_whole_step_against_the_restatement_and_twice():
    """(2, 25, 2) at B = 37 with PER weights and n-step discounts: every value, every gradient and the moved targets against the restatement;
    two runs from the same parameters give equal bits."""
    c = TC.case(TC.STEP)
    ent = TC.ent_of(c)
    got, again = _step(_head(c), c), _step(_head(c), c)
    assert not MG.differing(got, again), "two runs of the whole step differ in their bits"
    _check("step target", got["target"], TC.target_ref(c, c["discounts"], ent))
    ref = TC.critic_loss_ref(c, got["target"].double().cpu().numpy(), c["weights"])
    _check("step critic_loss", got["critic_loss"], ref["loss"])
    _check("step td", got["td"], ref["td_abs"])
    assert set(got["grad_critic"]) == set(TC.critic_names(c["arch"], 2))
    _check_grads("step critic_loss", got["grad_critic"], ref["grad"])
    ref = TC.actor_loss_ref(c, ent)
    _check("step actor_loss", got["actor_loss"], ref["loss"])
    _check("step log_prob", got["logp"], ref["log_prob"])
    grads = dict(got["grad_actor"], x=got["dx"])
    _check_grads("step actor_loss", grads, ref["grad"])
    moved = TC.polyak_ref(c)
    assert set(moved) == set(got["moved"])
    for k, v in moved.items():
        _check("step moved " + k, got["moved"][k], v)
        assert not torch.equal(got["moved"][k].cpu(), torch.from_numpy(c["params"][k])), k


@pytest.mark.parametrize("source", ["tqc", "ens3"])
def test_one_quantile_is_the_ensembles_critic(source):
    """n_quantiles = 1 on the weights of a SACEnsembleHead of the same N: `quantiles` has the bits of its `q_values` (the same tile code at
    width 1), for the grid's (1, 1, 0) case and for the ensemble's own N = 3 case."""
    if source == "tqc":
        c = TC.case(TC.ANCHOR)
        Fd, pi, qf, A = c["arch"]
    else:
        c = EC.case("a64_n3_b17")
        Fd, pi, qf, A = c["arch"]
    N = c["n_critics"]
    net_arch = dict(pi=list(pi), qf=list(qf))
    sd = {k: torch.from_numpy(np.asarray(v)) for k, v in c["params"].items()}
    tqc = m3l_amd.TQCHead(Fd, A, net_arch=net_arch, n_critics=N, n_quantiles=1, top_quantiles_to_drop_per_net=0)
    ens = m3l_amd.SACEnsembleHead(Fd, A, net_arch=net_arch, n_critics=N)
    tqc.load_state_dict(sd, strict=True)
    ens.load_state_dict(sd, strict=True)
    tqc, ens = tqc.to(DEV), ens.to(DEV)
    x, a = _t(c, "x"), _t(c, "a_replay")
    with torch.no_grad():
        for target in (False, True):
            z, q = tqc.quantiles(x, a, target=target), ens.q_values(x, a, target=target)
            assert z.shape == (N, x.shape[0], 1) and torch.equal(z[..., 0], q), f"target={target}: the bits differ from SACEnsembleHead.q_values"
    # with one quantile and nothing dropped the target is the pooled, sorted N values: at N = 1 the ensemble's target_q (another kernel's
    # epilogue: asserted to the bound, not to the bit)
    if N == 1:
        args = (_t(c, "x_next"), _t(c, "rewards"), _t(c, "dones"), c["gamma"])
        kw = dict(ent_coef=0.2, noise=_t(c, "noise_next"))
        _check("one quantile: target against the ensemble's target_q", tqc.td_target(*args, **kw)[:, 0], ens.td_target(*args, **kw).double().cpu().numpy())


def _contract_step(head, c, g):
    """Every new entry point once: quantiles forward and backward, the TD target in both gamma forms, the critic loss in both forms with their
    backwards, the actor loss and its backward, the Polyak update."""
    _clear(head)
    x, a = _t(c, "x").requires_grad_(True), _t(c, "a_replay")
    target = head.td_target(_t(c, "x_next"), _t(c, "rewards"), _t(c, "dones"), _t(c, "discounts"), log_ent_coef=_log_ent(c), noise=_t(c, "noise_next"))
    full = head.td_target(_t(c, "x_next"), _t(c, "rewards"), _t(c, "dones"), c["gamma"], ent_coef=0.2, noise=_t(c, "noise_next"))
    g.check("after td_target")
    loss, td = head.critic_loss(x, a, target, weights=_t(c, "weights"), return_td_errors=True)
    g.check("after critic_loss")
    loss.backward()
    g.check("after critic_loss.backward")
    out = dict(target=target, full=full, critic_loss=loss.detach(), td=td, grad_critic={n: p.grad.clone() for n, p in head.named_parameters() if p.grad is not None})
    plain = head.critic_loss(x, a, full)
    plain.backward()
    g.check("after the unweighted critic_loss")
    out["grad_critic_plain"] = {n: p.grad.clone() for n, p in head.named_parameters() if p.grad is not None}
    _clear(head)
    al, logp = head.actor_loss(x, ent_coef=0.2, noise=_t(c, "noise_pi"))
    g.check("after actor_loss")
    al.backward()
    g.check("after actor_loss.backward")
    out.update(actor_loss=al.detach(), logp=logp, grad_actor={n: p.grad.clone() for n, p in head.named_parameters() if p.grad is not None}, dx=x.grad)
    head.polyak_update(c["tau"])
    g.check("after polyak_update")
    out["moved"] = {n: p.detach().clone() for n, p in head.named_parameters() if n.startswith("critic_target.")}
    return out


@pytest.mark.parametrize("name", CONTRACT)
def test_memory_contract(monkeypatch, name):
    """Every new entry point under guarded, poisoned allocations: no write outside a buffer, no read of stale workspace, scratch, padding or
    outputs, the bits of the unguarded run, and every workspace request sized by the *_ws_bytes call in front of it."""
    c = TC.case(name)
    params = {k: torch.from_numpy(np.asarray(v)).to(DEV) for k, v in c["params"].items()}
    head = _head(c)

    def work(g):
        with torch.no_grad():
            for n, p in head.named_parameters():
                p.copy_(params[n])          # the Polyak update of the run before is undone
        return _contract_step(head, c, g)
    counts = MG.run_contract(monkeypatch, work)
    # workspaces: per critic loss the critic node's and the loss's scratch, and for the actor loss the actor node's and the critic node's
    assert counts[0] == counts[1] and counts[0][0] == 6, counts


@pytest.mark.parametrize("name", ["f16_a1_q32_n3q5d4_b1", "f16_a7_q32_n10q25d2_b17"])
def test_no_grad_calls_take_no_workspace(monkeypatch, name):
    c = TC.case(name)
    head = _head(c)
    x, a, noise = _t(c, "x"), _t(c, "a_replay"), _t(c, "noise_pi")

    def no_grad(g):
        with torch.no_grad():
            out = [head.quantiles(x, a), head.quantiles(x, a, target=True), head(x, noise=noise)]
        out.append(head.td_target(x, _t(c, "rewards"), _t(c, "dones"), 0.99, ent_coef=0.2, noise=noise))
        g.check("after the no_grad calls")
        return {"out": out}

    def grad(g):
        z = head.quantiles(x, a)
        g.check("after the grad-mode call")
        return {"out": [z.detach()]}
    sized = []
    lib = L.lib()
    real = lib.m3l_tqc_ws_bytes
    monkeypatch.setattr(lib, "m3l_tqc_ws_bytes", lambda *args: sized.append(1) or real(*args))
    counts = MG.run_contract(monkeypatch, no_grad, need_ws=False)
    assert all(n_ws == 0 for n_ws, _ in counts) and not sized, (counts, len(sized))
    counts = MG.run_contract(monkeypatch, grad)
    assert all(n_ws == 1 for n_ws, _ in counts) and len(sized) == 3
    frozen = _head(c).requires_grad_(False)          # nothing requires a gradient: no workspace in grad mode either
    sized.clear()
    z = frozen.quantiles(x.clone().requires_grad_(True), a)          # the features never do, for the critics
    assert not sized and not z.requires_grad
    z = frozen.quantiles(x, a.clone().requires_grad_(True))          # the actions do
    assert len(sized) == 1 and z.requires_grad


def test_refusals_that_need_a_device():
    c = TC.case("f16_a7_q48x32_n3q5d4_b37")
    head = _head(c)
    x, a, v = _t(c, "x"), _t(c, "a_replay"), _t(c, "rewards")
    t = torch.zeros(37, 3, device=DEV)
    for call in (lambda: head(x.cpu()), lambda: head.quantiles(x, a.cpu()), lambda: head.quantiles(x.cpu(), a), lambda: head.td_target(x, v.cpu(), v, 0.99, ent_coef=0.1),
                 lambda: head.critic_loss(x, a, t.cpu()), lambda: head.critic_loss(x, a, t, weights=v.cpu()), lambda: head.actor_loss(x.cpu(), ent_coef=0.1),
                 lambda: TQ.actor_loss_from(v.cpu(), torch.zeros(3, 37, 5, device=DEV), ent_coef=0.1)):
        with pytest.raises(m3l_amd.M3LError):
            call()
    dev = lambda *s, **k: torch.zeros(*s, device=DEV, **k)      # noqa: E731
    for call in (lambda: head.td_target(x, v, v, 0.99), lambda: head.td_target(x, v, v, 0.99, ent_coef=0.1, log_ent_coef=dev(1)), lambda: head.td_target(x, v[:2], v, 0.99, ent_coef=0.1),
                 lambda: head.td_target(x, v, v, dev(36), ent_coef=0.1), lambda: head.quantiles(x, a[:2]), lambda: head.quantiles(x, dev(37, 6)),
                 lambda: head.critic_loss(x, a, dev(37, 4)), lambda: head.critic_loss(x, a, dev(37)), lambda: head.critic_loss(x, a, dev(36, 3)),
                 lambda: head.critic_loss(x, a, t, weights=v[:2]), lambda: head.critic_loss(x, a, t.double()),
                 lambda: TQ.critic_loss_from(dev(11, 37, 5), t), lambda: TQ.critic_loss_from(dev(3, 37, 65), t), lambda: TQ.critic_loss_from(dev(3, 37), t),
                 lambda: TQ.critic_loss_from(dev(3, 37, 5), dev(37, 513)), lambda: TQ.actor_loss_from(v[:2], dev(3, 37, 5), ent_coef=0.1)):
        with pytest.raises(ValueError):
            call()
    # the C ABI refuses what the header excludes, with the reason, and writes nothing
    lib = L.lib()
    p = head.params()
    arch = TQ._arch(16, p)
    z = torch.full((3, 37, 5), 7.0, device=DEV)
    for change, why in ((dict(n_quantiles=0), "n_quantiles"), (dict(n_quantiles=65), "n_quantiles"), (dict(top_quantiles_to_drop=5), "top_quantiles_to_drop"),
                        (dict(B=0), "B >= 1")):
        d = TQ._desc(arch, p, actor=p.actor_flat(), critic=p.critic_flat())
        B = change.pop("B", 37)
        for k, val in change.items():
            setattr(d, k, val)
        assert lib.m3l_tqc_critic_fwd(C.byref(d), B, L.ptr(x), L.ptr(a), None, L.ptr(z), None) != 0 and why in L.last_error(), L.last_error()
        assert lib.m3l_tqc_td_target(C.byref(d), B, L.ptr(x), None, L.ptr(v), L.ptr(v), None, 0.99, 0.1, None, L.ptr(z), None) != 0
    d = TQ._desc(arch, p, actor=p.actor_flat(), critic=p.critic_flat())
    d.ens.n_critics = 11
    assert lib.m3l_tqc_critic_fwd(C.byref(d), 37, L.ptr(x), L.ptr(a), None, L.ptr(z), None) != 0 and "n_critics" in L.last_error()
    assert lib.m3l_tqc_critic_fwd(C.byref(TQ._desc(arch, p, actor=p.actor_flat())), 37, L.ptr(x), L.ptr(a), None, L.ptr(z), None) != 0 and "null" in L.last_error()
    ws = torch.zeros(1024, device=DEV)
    assert lib.m3l_tqc_critic_loss_fwd(L.ptr(z), L.ptr(t), None, 3, 37, 5, 513, L.ptr(ws), L.ptr(z), L.ptr(z), None, None) != 0 and "K=513" in L.last_error()
    assert lib.m3l_tqc_critic_loss_fwd(L.ptr(z), L.ptr(t), None, 3, 37, 5, 3, None, L.ptr(z), L.ptr(z), None, None) != 0 and "null" in L.last_error()
    assert lib.m3l_tqc_critic_loss_fwd(L.ptr(z), L.ptr(t), None, 11, 37, 5, 3, L.ptr(ws), L.ptr(z), L.ptr(z), None, None) != 0
    assert lib.m3l_tqc_actor_loss_fwd(L.ptr(v), L.ptr(z), 3, 37, 65, 0.1, None, L.ptr(z), L.ptr(z), None) != 0 and "n_quantiles" in L.last_error()
    torch.cuda.synchronize()
    assert bool((z == 7.0).all()) and bool((ws == 0).all())


@pytest.mark.parametrize("name", ["f32_a7_q32_n2q25d2_b17", "f16_a1_nohid_n2q64d0_b17"])
def test_a_nan_quantile_stays_in_range(monkeypatch, name):
    """A NaN in one target critic's last bias makes one pooled value of every row NaN.  td_target returns, no guard byte changes under either
    fill, every output element is written, and the result is the restatement's with torch.sort's NaN-last order: with d = 2 the NaN is among
    the N d dropped values and every row is finite; with d = 0 it is the last kept column of every row.  Nothing here can address out of
    range: the rank count compares integer keys, and every rank lies in [0, pool)."""
    base = TC.case(name)
    params = dict(base["params"])
    key = f"critic_target.qf1.{2 * len(base['arch'][2])}.bias"
    params[key] = params[key].copy()
    params[key][3] = np.nan
    c = dict(base, params=params)
    head = _head(c)
    ent = TC.ent_of(c)
    ref = TC.target_ref(c, c["gamma"], ent)
    outs = []
    for fill in MG.FILLS:
        with MG.MemGuard(monkeypatch, fill) as g:
            got = head.td_target(_t(c, "x_next"), _t(c, "rewards"), _t(c, "dones"), c["gamma"], ent_coef=ent, noise=_t(c, "noise_next"))
            g.check("after td_target with a NaN quantile")
            assert g.n_tensors > 0
            outs.append(got.clone())
    assert torch.equal(torch.isnan(outs[0]), torch.isnan(outs[1])) and torch.equal(torch.nan_to_num(outs[0]), torch.nan_to_num(outs[1]))
    nan = np.isnan(ref)
    assert np.array_equal(torch.isnan(outs[0]).cpu().numpy(), nan)
    if c["drop"] == 0:
        assert nan[:, -1].all() and not nan[:, :-1].any()
    else:
        assert not nan.any()
    _check(name + " target beside the NaN", torch.nan_to_num(outs[0]), np.nan_to_num(ref))
