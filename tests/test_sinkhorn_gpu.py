"""GPU checks of the Sinkhorn-Knopp teacher assignment: the column-pass kernels (m3l_op_sk_*), DINOLoss.sinkhorn_knopp_teacher /
softmax_center_teacher / forward(centering="sinkhorn_knopp") and VTDINO(centering="sinkhorn_knopp").

Yardsticks.  Recorded cases: the float64 run of the reference's own sinkhorn_knopp_teacher (tests/golden/make_golden_sinkhorn.py).  Other
shapes: `sinkhorn_log_domain` of test_sinkhorn_cpu.py in float64, which the CPU test pins to those recorded results to 1e-12.  The step:
the float64 run of the reference's VTDINO with its teacher-probability call routed to sinkhorn_knopp_teacher (vtdino_sk_step*.npz).

Bound of the probabilities: 4 x `log32_err`, the largest elementwise relative error of a float32 torch run of the same log-domain
arithmetic on the CPU against float64 (recorded per case, or computed here for the shapes made here).  The yardstick of the error is that
CPU float32 run, not the kernels; the factor covers the kernels' v_exp_f32 and their summation order.  The rounding the bound scales with
is that of z = l / tt (|z| up to 37 at tt = 0.04: 37 * 2^-24 ~ 2e-6 absolute in the exponent, the same relative in the probability).
Wide-range case (2 * randn at tt = 0.04, probabilities down to 1e-128): the elementwise relative error is ill-conditioned, so error and
log32_err are both measured relative to the row's largest probability.
"""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import m3l_amd
import memguard as MG
from m3l_amd import _lib as L
from m3l_amd import dino as D
from test_sinkhorn_cpu import sinkhorn_cases, sinkhorn_log_domain
from test_vtdino_cpu import _z, build_step_module, load_step_params

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROW_SUM_TOL = 1e-4          # the loss kernels' lse bar (tests/test_vtdino_gpu.py)


def _stream():
    return torch.cuda.current_stream().cuda_stream


def cosine_logits(rows, K, seed, dim=32):
    """normalize(x) @ (normalize(W) * g).T with g in [0.5, 1.5]: what the weight-normalised prototype layer gives, |l| <= 1.5."""
    g = torch.Generator().manual_seed(seed)
    x = F.normalize(torch.randn(rows, dim, generator=g), dim=-1)
    W = F.normalize(torch.randn(K, dim, generator=g), dim=-1) * (0.5 + torch.rand(K, 1, generator=g))
    return (x @ W.t()).contiguous()


def _rel_err(got, ref64):
    return float(((got.double() - ref64).abs() / ref64).max())


def _log32_err(logits, tt, n=3):
    """float32 CPU run of the log-domain iteration against its float64 run -> (largest relative error, float64 probabilities)."""
    T64, _ = sinkhorn_log_domain(logits, tt, n, torch.float64)
    T32, _ = sinkhorn_log_domain(logits, tt, n, torch.float32)
    return _rel_err(T32, T64), T64


def _row_sum_err(T):
    return float((T.double().sum(dim=-1) - 1.0).abs().max())


RELATIVE_CASES = ["cos_b3_t04", "cos_b3_t07", "cos_b35_t07", "cos_b3_t04_it1"]


# ---- 1. recorded cases ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", RELATIVE_CASES)
def test_recorded_cases_against_the_reference_float64_run(name):
    """Error against float64 within 4 x the case's recorded float32 error, rows sum to one, two runs the same bits, and within that bound plus
    the reference's own float32 error of the reference's float32 output; the centre buffers are not touched."""
    c = sinkhorn_cases()[name]
    assert c["measure"] == "relative" and c["ref32_finite"]
    crit = m3l_amd.DINOLoss(c["shape"][-1]).to(DEV)
    T = c["logits"].view(c["shape"]).to(DEV)
    a = crit.sinkhorn_knopp_teacher(T, c["tt"], n_iterations=c["n"])
    b = crit.sinkhorn_knopp_teacher(T, c["tt"], n_iterations=c["n"])
    assert tuple(a.shape) == (c["shape"][0] * c["shape"][1], c["shape"][2]) and a.dtype == torch.float32
    f64, ref32 = torch.from_numpy(c["f64"]), torch.from_numpy(c["ref32"])
    bound = 4.0 * c["log32_err"]
    err, err_ref, rs = _rel_err(a.cpu(), f64), float(((a.cpu().double() - ref32.double()).abs() / f64).max()), _row_sum_err(a.cpu())
    print(f"sinkhorn {name}: rel err vs float64 {err:.3e} (bound {bound:.3e})  vs the reference's float32 run {err_ref:.3e} "
          f"(bound {bound + c['ref32_err']:.3e})  row sums within {rs:.2e}")
    assert err <= bound
    assert rs <= ROW_SUM_TOL
    assert torch.equal(a, b), "two runs on the same input differ"
    assert err_ref <= bound + c["ref32_err"]
    assert float(crit.center.abs().max()) == 0.0 and crit.updated is True and crit.async_batch_center is None


# ---- 2. row ranges -------------------------------------------------------------------------------------------------------------------------
RANGE_SHAPES = [(70, 1000), (1030, 1000), (70, 4096)]


def test_row_range_shapes_cover_more_than_one_range_with_a_ragged_last_one():
    """rows % splits != 0 means no cut into `splits` equal ranges exists: the last range is shorter than the others."""
    lib = L.lib()
    splits = {s: lib.m3l_op_sk_row_splits(*s) for s in RANGE_SHAPES}
    print("row ranges:", splits)
    assert any(n > 1 and rows % n != 0 for (rows, _), n in splits.items()), splits
    assert all(lib.m3l_op_sk_ws_bytes(rows, K) >= n * K * 8 for (rows, K), n in splits.items())


@pytest.mark.parametrize("rows,K", RANGE_SHAPES)
def test_row_ranges_against_float64_restatement(rows, K):
    """(70, 1000) and (70, 4096) run 18 ranges of 4 rows with 2 in the last, (1030, 1000) 61 ranges of 17 with 10 in the last."""
    tt = 0.04
    logits = cosine_logits(rows, K, seed=rows + K)
    log32, T64 = _log32_err(logits, tt)
    crit = m3l_amd.DINOLoss(K).to(DEV)
    a = crit.sinkhorn_knopp_teacher(logits.to(DEV), tt)
    b = crit.sinkhorn_knopp_teacher(logits.to(DEV), tt)
    err, rs = _rel_err(a.cpu(), T64), _row_sum_err(a.cpu())
    print(f"sinkhorn rows {rows} K {K} ({L.lib().m3l_op_sk_row_splits(rows, K)} row ranges): rel err {err:.3e} (bound {4 * log32:.3e}, "
          f"CPU float32 {log32:.3e})  row sums within {rs:.2e}")
    assert err <= 4.0 * log32
    assert rs <= ROW_SUM_TOL
    assert torch.equal(a, b)


# ---- 3. wide range -------------------------------------------------------------------------------------------------------------------------
def test_wide_range_logits_stay_finite_where_the_reference_float32_run_overflows():
    """2 * randn at tt = 0.04: z reaches 200, the reference's float32 exp overflows; the kernels never form exp(z)."""
    c = sinkhorn_cases()["wide_b3_t04"]
    assert c["measure"] == "rowmax" and not c["ref32_finite"]
    crit = m3l_amd.DINOLoss(c["shape"][-1]).to(DEV)
    a = crit.sinkhorn_knopp_teacher(c["logits"].view(c["shape"]).to(DEV), c["tt"], n_iterations=c["n"]).cpu()
    f64 = torch.from_numpy(c["f64"])
    bound = 4.0 * c["log32_err"]
    err = float(((a.double() - f64).abs() / f64.amax(dim=1, keepdim=True)).max())
    print(f"sinkhorn wide range: error {err:.3e} of the row maximum (bound {bound:.3e})  row sums within {_row_sum_err(a):.2e}")
    assert bool(torch.isfinite(a).all())
    assert err <= bound
    assert _row_sum_err(a) <= ROW_SUM_TOL


# ---- 4. virtual ranks ----------------------------------------------------------------------------------------------------------------------
def _virtual_ranks(logits, tt, nparts, n_iterations=3):
    """The iteration through the C ABI with the rows cut into `nparts` contiguous blocks, each block's column pairs computed on its own (as a
    rank would) and merged by m3l_op_sk_colcombine in block order; the row pass runs over all rows."""
    lib = L.lib()
    rows, K = logits.shape
    cuts = [rows * i // nparts for i in range(nparts + 1)]
    parts = torch.empty(nparts, K, 2, device=DEV)
    center = torch.empty(K, device=DEV)
    stats = None
    for it in range(n_iterations):
        for i in range(nparts):
            r0, n = cuts[i], cuts[i + 1] - cuts[i]
            ws = torch.empty(lib.m3l_op_sk_ws_bytes(n, K), dtype=torch.uint8, device=DEV)
            L.check(lib.m3l_op_sk_colstats(L.ptr(logits[r0:]), n, K, 1.0 / tt, L.ptr(stats[r0:]) if stats is not None else None, L.ptr(ws),
                                           L.ptr(parts[i]), _stream()), "m3l_op_sk_colstats")
        L.check(lib.m3l_op_sk_colcombine(L.ptr(parts), nparts, K, tt, L.ptr(center), _stream()), "m3l_op_sk_colcombine")
        stats = D._row_stats(logits, rows, K, center, 1.0 / tt)
    probs = torch.empty(rows, K, device=DEV)
    L.check(lib.m3l_op_sk_probs(L.ptr(logits), rows, K, L.ptr(center), 1.0 / tt, L.ptr(stats), L.ptr(probs), _stream()), "m3l_op_sk_probs")
    return probs, center


@pytest.mark.parametrize("nparts", [2, 3])
def test_virtual_ranks_through_the_c_abi(nparts):
    """Blocks of 35 + 35 and of 23 + 23 + 24 rows, merged with nparts = 2 and 3."""
    rows, K, tt = 70, 1000, 0.04
    logits = cosine_logits(rows, K, seed=rows + K)
    log32, T64 = _log32_err(logits, tt)
    lg = logits.to(DEV)
    a, ca = _virtual_ranks(lg, tt, nparts)
    b, cb = _virtual_ranks(lg, tt, nparts)
    err = _rel_err(a.cpu(), T64)
    print(f"sinkhorn {nparts} virtual ranks: rel err {err:.3e} (bound {4 * log32:.3e})")
    assert err <= 4.0 * log32
    assert _row_sum_err(a.cpu()) <= ROW_SUM_TOL
    assert torch.equal(a, b) and torch.equal(ca, cb)


# ---- 5. loss -------------------------------------------------------------------------------------------------------------------------------
def _sk_loss_restated(S, T, ts, tt, n=3):
    """float64, pairwise, with Sinkhorn-Knopp targets over the (Q B) teacher rows."""
    Q, B, K = T.shape
    probs = sinkhorn_log_domain(T.reshape(Q * B, K), tt, n)[0].view(Q, B, K)
    total = 0
    for p in range(S.shape[0]):
        lsm = torch.log_softmax(S[p] / ts, dim=-1)
        for q in range(Q):
            total = total - torch.sum(probs[q] * lsm, dim=-1).mean()
    return total


@pytest.mark.parametrize("P,Q,B,K", [(3, 2, 3, 1000), (5, 2, 5, 4096)])
def test_loss_with_sinkhorn_targets_and_softmax_center_teacher(P, Q, B, K):
    """Teacher: cosine logits; student: 1.5 * randn.  A centre update is pending when the Sinkhorn-Knopp loss is called and must still be
    pending afterwards; softmax_center_teacher then applies it."""
    g = torch.Generator().manual_seed(K + P)
    ts, tt = 0.1, 0.04
    S64 = (1.5 * torch.randn(P, B, K, generator=g)).double().requires_grad_(True)
    T32 = cosine_logits(Q * B, K, seed=K).view(Q, B, K)
    ref = _sk_loss_restated(S64, T32.double(), ts, tt)
    ref.backward()
    crit = m3l_amd.DINOLoss(K, student_temp=ts).to(DEV)
    prev = cosine_logits(Q * B, K, seed=K + 1).view(Q, B, K).to(DEV)
    crit.update_center(prev)                              # a pending centre update that the Sinkhorn-Knopp call must leave pending
    pending = crit.async_batch_center
    before = (crit.center.clone(), pending.clone())
    S = S64.detach().float().to(DEV).requires_grad_(True)
    loss = crit(S, T32.to(DEV), tt, centering="sinkhorn_knopp")
    loss.backward()
    assert crit.updated is False and crit.async_batch_center is pending
    assert torch.equal(crit.center, before[0]) and torch.equal(pending, before[1])
    rel = abs(float(loss) - float(ref)) / abs(float(ref))
    gerr = float((S.grad.cpu().double() - S64.grad).abs().max() / S64.grad.abs().max())
    print(f"sinkhorn loss P={P} Q={Q} B={B} K={K}: loss rel {rel:.2e}  dS {gerr:.2e} of max")
    assert rel <= 1e-4 and gerr <= 1e-4
    # softmax_center_teacher applies the pending update, then softmax((T - center) / tt)
    probs = crit.softmax_center_teacher(T32.to(DEV), tt)
    assert crit.updated is True and float(crit.center.abs().max()) > 0
    z64 = (T32.double().view(Q * B, K) - crit.center.cpu().double()) / tt
    z32 = (T32.view(Q * B, K) - crit.center.cpu()) / tt
    p64 = torch.exp(z64 - torch.logsumexp(z64, dim=-1, keepdim=True))
    log32 = _rel_err(torch.exp(z32 - torch.logsumexp(z32, dim=-1, keepdim=True)), p64)
    err = _rel_err(probs.cpu(), p64)
    print(f"softmax_center_teacher: rel err {err:.3e} (bound {4 * log32:.3e})")
    want_center = (before[0].cpu() * crit.center_momentum + (before[1].cpu() / (Q * B)) * (1 - crit.center_momentum))
    assert torch.allclose(crit.center.cpu(), want_center, rtol=1e-6, atol=1e-7)
    assert tuple(probs.shape) == (Q * B, K) and err <= 4.0 * log32 and _row_sum_err(probs.cpu()) <= ROW_SUM_TOL


# ---- 6. step -------------------------------------------------------------------------------------------------------------------------------
def _max_rel(got, ref):
    return float(np.abs(got - ref).max()) / max(1e-30, float(np.abs(ref).max()))


def _rel_l2(got, ref):
    return float(np.linalg.norm((got - ref).ravel())) / max(1e-30, float(np.linalg.norm(ref.ravel())))


@pytest.mark.parametrize("dt", ["fp32", "bf16"])
def test_two_steps_with_sinkhorn_targets_against_reference_fixture(dt):
    """The recording scheme and bounds of test_vtdino_gpu.py::test_two_steps_against_reference_fixture (fp32: loss 1e-4, gradients 2e-3 of
    their largest entry; bf16: twice the recorded emulation error), with the parameters, inputs and masks of vtdino_step.npz.
    The centre stays zero and nothing is left pending."""
    z, zk = _z("vtdino_step.npz"), _z("vtdino_sk_step.npz")
    model = build_step_module(z, compute_dtype=dt, centering="sinkhorn_knopp")
    load_step_params(model, z)
    model = model.to(DEV)
    x = {k: torch.from_numpy(z["input/" + k]).to(DEV) for k in ("image", "tactile1", "tactile2")}
    lr = float(z["meta/lr"])
    for s in (1, 2):
        zs = _z(f"vtdino_sk_step_s{s}.npz")
        for p in model.parameters():
            p.grad = None
        out = model.training_step(x, s - 1)
        out["loss"].backward()
        torch.cuda.synchronize()
        ref_loss = float(zk[f"step{s}/loss"])
        loss_rel = abs(out["ssl_loss"] - ref_loss) / abs(ref_loss)
        named = dict(model.student_encoder.named_parameters())
        grad_names = [k[len("grad/"):] for k in zs.files if k.startswith("grad/")]
        emax = {n: _max_rel(named[n].grad.cpu().numpy(), zs["grad/" + n]) for n in grad_names}
        el2 = {n: _rel_l2(named[n].grad.cpu().numpy(), zs["grad/" + n]) for n in grad_names}
        s_err = float(np.abs(model.last["student_logits"].cpu().numpy() - zs["student_logits"]).max())
        t_err = float(np.abs(model.last["teacher_logits"].cpu().numpy() - zs["teacher_logits"]).max())
        if dt == "fp32":
            b_loss, b_max, b_l2 = 1e-4, 2e-3, None
            b_s = b_t = 1e-4 + 1e-3 * float(np.abs(zs["student_logits"]).max())
        else:
            pre = f"bf16emu/step{s}/"
            b_loss, b_max, b_l2 = 2 * float(zk[pre + "loss_rel"]), 2 * float(zk[pre + "grad_max_rel"].max()), 2 * float(zk[pre + "grad_rel_l2"].max())
            b_s, b_t = 2 * float(zk[pre + "student_logits_max_abs"]), 2 * float(zk[pre + "teacher_logits_max_abs"])
        worst = max(emax, key=emax.get)
        print(f"[{dt}] sinkhorn step {s}: loss {out['ssl_loss']:.6f} ref {ref_loss:.6f} rel {loss_rel:.3e} (bound {b_loss:.3e})  grad max-rel worst "
              f"{emax[worst]:.3e} at {worst} (bound {b_max:.3e})  rel-L2 worst {max(el2.values()):.3e} (bound {b_l2})  logits max-abs student "
              f"{s_err:.3e} (bound {b_s:.3e}) teacher {t_err:.3e} (bound {b_t:.3e})")
        assert loss_rel <= b_loss, (s, loss_rel, b_loss)
        assert s_err <= b_s and t_err <= b_t, (s, s_err, b_s, t_err, b_t)
        for n in grad_names:
            assert emax[n] <= b_max, (s, n, emax[n], b_max)
            if b_l2 is not None:
                assert el2[n] <= b_l2, (s, n, el2[n], b_l2)
        assert all(p.grad is None for p in model.teacher_encoder.parameters()), "the teacher received a gradient"
        with torch.no_grad():
            for p in model.student_encoder.parameters():
                if p.grad is not None:
                    p.sub_(lr * p.grad)
        model.on_train_batch_end(out, x, s - 1)
        assert float(model.dino_loss.center.abs().max()) == 0.0 and model.dino_loss.updated is True
        assert model.dino_loss.async_batch_center is None


def test_default_centering_still_gives_the_recorded_loss():
    z = _z("vtdino_step.npz")
    model = build_step_module(z, compute_dtype="fp32")
    assert model.centering == "centering"
    load_step_params(model, z)
    model = model.to(DEV)
    x = {k: torch.from_numpy(z["input/" + k]).to(DEV) for k in ("image", "tactile1", "tactile2")}
    out = model.training_step(x, 0)
    ref = float(z["step1/loss"])
    assert abs(out["ssl_loss"] - ref) <= 1e-4 * abs(ref)
    assert model.dino_loss.updated is False and model.dino_loss.async_batch_center is not None
    assert abs(ref - float(_z("vtdino_sk_step.npz")["step1/loss"])) > 1e-3 * abs(ref), "the two centring modes recorded the same loss"


# ---- 7. full size --------------------------------------------------------------------------------------------------------------------------
def test_full_size_runs_and_repeats():
    Q, B, K, tt = 2, 32, 65536, 0.04
    logits = cosine_logits(Q * B, K, seed=7).view(Q, B, K).to(DEV)
    crit = m3l_amd.DINOLoss(K).to(DEV)
    ca = crit.sinkhorn_knopp_center(logits, tt)
    cb = crit.sinkhorn_knopp_center(logits, tt)
    assert tuple(ca.shape) == (K,) and ca.dtype == torch.float32 and torch.equal(ca, cb)
    T = crit.sinkhorn_knopp_teacher(logits, tt)
    assert tuple(T.shape) == (Q * B, K) and bool(torch.isfinite(T).all())
    rs = float((T.double().sum(dim=-1) - 1.0).abs().max())
    cs = float((T.double().sum(dim=0) * K / (Q * B) - 1.0).abs().max())
    print(f"sinkhorn full size: {L.lib().m3l_op_sk_row_splits(Q * B, K)} row ranges, row sums within {rs:.2e}, column sums x K / rows within {cs:.2e} of one")
    assert rs <= ROW_SUM_TOL


# ---- 8. memory contract --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("Q,B,K", [(2, 35, 1000), (2, 5, 8192)])
def test_memory_contract(monkeypatch, Q, B, K):
    P = 3
    g0 = torch.Generator().manual_seed(K)
    teacher = cosine_logits(Q * B, K, seed=B).view(Q, B, K).to(DEV)
    student = (1.5 * torch.randn(P, B, K, generator=g0)).to(DEV)

    def work(g):
        crit = m3l_amd.DINOLoss(K).to(DEV)
        probs = crit.sinkhorn_knopp_teacher(teacher, 0.04)
        g.check("after sinkhorn_knopp_teacher")
        s = student.clone().requires_grad_(True)
        loss = crit(s, teacher, 0.04, centering="sinkhorn_knopp")
        g.check("after the forward")
        loss.backward()
        g.check("after the backward")
        return {"probs": probs, "loss": loss, "dS": s.grad, "center": crit.sinkhorn_knopp_center(teacher, 0.04, n_iterations=1)}
    MG.run_contract(monkeypatch, work)
