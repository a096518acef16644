"""GPU checks of the iBOT patch loss (m3l_op_ibot_loss / _grad / _center_sum, m3l_amd.iBOTPatchLoss, VTDINO(ibot=True)).

Yardsticks: the float64 restatement of tests/ibot_cases.py, which test_ibot_cpu.py pins to the results recorded from the reference's own
iBOTPatchLoss (loss 1e-12, dS 1e-13, Sinkhorn-Knopp probabilities 2e-14), and the two step fixtures recorded from the reference's VTDINO step with
the patch term added as its DINOv2 algorithm adds it (tests/golden/make_golden_ibot.py).  Bounds are those of test_vtdino_gpu.py for loss kernels:
loss 1e-4 relative, f32 dS^T within 1e-4 of its largest entry, bf16 dS^T within 2^-8 relative plus 2e-4 of the largest entry, `pending` and centre
rtol 1e-5 / atol 1e-5; steps: fp32 loss 1e-4 relative and gradients within 2e-3 of their largest entry, bf16 twice the recorded errors of the
bf16-operand emulation."""
from functools import lru_cache, partial

import numpy as np
import pytest
import torch

import ibot_cases as IC
import m3l_amd
import memguard as MG
from m3l_amd import _lib as L
from m3l_amd import dino as D
from test_ibot_cpu import restated
from test_vtdino_cpu import _z, build_step_module

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TS, TT, MOM = IC.STUDENT_TEMP, IC.TEACHER_TEMP, IC.MOMENTUM
INV_TS, INV_TT = 1.0 / TS, 1.0 / TT
F32, BF16 = 0, 1


def _stream():
    return torch.cuda.current_stream().cuda_stream


@lru_cache(maxsize=None)
def _case(shape):
    """(S, T, centre) on the device and the float64 results with the centre, computed once per shape."""
    if shape in IC.RECORDED:
        (S, T, c), r, _, _ = restated(shape)
    else:
        S, T, c = IC.inputs(*shape)
        r = IC.ibot_f64(S, T, c, IC.SHAPES[shape])
    return (S.to(DEV), T.to(DEV), c.to(DEV)), r


def _stats(S, T, c):
    Q, R, K = S.shape
    return D._row_stats(S, Q * R, K, None, INV_TS), D._row_stats(T, Q * R, K, c, INV_TT)


def _loss(S, T, c, stats):
    Q, R, K = S.shape
    lib = L.lib()
    loss = torch.empty(1, dtype=torch.float32, device=DEV)
    ws = torch.empty(int(lib.m3l_op_ibot_ws_bytes(R, K)), dtype=torch.uint8, device=DEV)
    rc = lib.m3l_op_ibot_loss(L.ptr(S), L.ptr(T), Q, R, K, L.ptr(c), INV_TS, INV_TT, L.ptr(stats[0]), L.ptr(stats[1]), L.ptr(ws), L.ptr(loss), _stream())
    assert rc == 0, L.last_error()
    return loss


def _grad(S, T, c, stats, dt, dloss=1.0):
    """-> dS^T (K, ldr) as the kernel left it in a buffer that held NaN."""
    Q, R, K = S.shape
    ldr = D._ld8(Q * R)
    dST = torch.full((K, ldr), float("nan"), dtype=torch.bfloat16 if dt == BF16 else torch.float32, device=DEV)
    g = torch.tensor([dloss], dtype=torch.float32, device=DEV)
    rc = L.lib().m3l_op_ibot_grad(dt, L.ptr(S), L.ptr(T), Q, R, K, L.ptr(c), INV_TS, INV_TT, L.ptr(stats[0]), L.ptr(stats[1]), L.ptr(g), L.ptr(dST), ldr,
                                  _stream())
    assert rc == 0, L.last_error()
    return dST


def _center_sum(T, n):
    lib = L.lib()
    K = T.shape[-1]
    rows = T.numel() // K
    pending = torch.empty(K, dtype=torch.float32, device=DEV)
    ws = torch.empty(int(lib.m3l_op_ibot_ws_bytes(rows, K)), dtype=torch.uint8, device=DEV)
    rc = lib.m3l_op_ibot_center_sum(L.ptr(T), rows, K, 1.0 / n, L.ptr(ws), L.ptr(pending), _stream())
    assert rc == 0, L.last_error()
    return pending


def _unT(dST, Q, R):
    return dST.t()[:Q * R].reshape(Q, R, -1).cpu().double().numpy()


def _check_grads(what, d32, d16, ref):
    gmax = float(np.abs(ref).max())
    e32 = float(np.abs(d32 - ref).max()) / gmax
    over16 = float((np.abs(d16 - ref) - (2.0 ** -8 * np.abs(ref) + 2e-4 * gmax)).max())
    print(f"[{what}] f32 dS^T err {e32:.2e} of the largest entry {gmax:.3e} (bound 1e-4)  bf16 dS^T worst excess over its bound {over16:.2e} (must be <= 0)")
    assert e32 <= 1e-4, (what, e32)
    assert over16 <= 0, (what, over16)


@pytest.mark.parametrize("shape", list(IC.SHAPES))
def test_kernels_against_the_float64_restatement(shape):
    """One row; one row past the old 255 limit; partial row and column tiles; several row tiles; the full prototype count.  Measured on an
    MI355X over the six shapes (EXPERIMENTS.md 5.10 lists each): loss 3.5e-9 to 9.5e-8 relative (bound 1e-4); f32 dS^T 4.4e-7 to 1.1e-6 of the largest
    entry (bound 1e-4); bf16 dS^T inside 2^-8 |ref| + 2e-4 max|ref| everywhere; pending at most 6.8e-7, centre at most 3.6e-8 absolute
    (rtol 1e-5 / atol 1e-5); two runs the same bits; pad columns exactly zero."""
    (S, T, c), r = _case(shape)
    Q, R, K = shape
    n = IC.SHAPES[shape]
    stats = _stats(S, T, c)
    loss, d32 = _loss(S, T, c, stats), _grad(S, T, c, stats, F32)
    loss_b, d32_b = _loss(S, T, c, stats), _grad(S, T, c, stats, F32)
    d16 = _grad(S, T, c, stats, BF16)
    torch.cuda.synchronize()
    npad = D._ld8(Q * R) - Q * R
    assert torch.equal(loss, loss_b) and torch.equal(d32[:, :Q * R], d32_b[:, :Q * R]), "two runs differ in their bits"
    assert bool((d32[:, Q * R:] == 0).all()) and bool((d16[:, Q * R:] == 0).all()), "pad columns are not exactly zero"
    loss_err = abs(float(loss) - r["loss"]) / abs(r["loss"])
    print(f"[{IC.case_name(*shape)}] loss {float(loss):.6f} ref {r['loss']:.6f} rel {loss_err:.2e} (bound 1e-4)  pad columns {npad}")
    assert loss_err <= 1e-4, loss_err
    _check_grads(IC.case_name(*shape), _unT(d32, Q, R), _unT(d16, Q, R), r["dS"])
    pending = _center_sum(T, n)
    center = c.clone()
    rc = L.lib().m3l_op_dino_center_apply(L.ptr(center), L.ptr(pending), K, MOM, 1 - MOM, float(Q * R // n), _stream())
    assert rc == 0, L.last_error()
    assert torch.equal(pending, _center_sum(T, n)), "two runs differ in their bits"
    print(f"[{IC.case_name(*shape)}] pending max err {np.abs(pending.cpu().numpy() - r['pending']).max():.2e}  centre max err "
          f"{np.abs(center.cpu().numpy() - r['center_after']).max():.2e} (rtol 1e-5 / atol 1e-5)")
    np.testing.assert_allclose(pending.cpu().numpy(), r["pending"], rtol=1e-5, atol=1e-5)
    np.testing.assert_allclose(center.cpu().numpy(), r["center_after"], rtol=1e-5, atol=1e-5)


def test_agrees_with_the_dino_kernels_where_both_can_run():
    Q, R, K = 2, 64, 1000
    S, T, c = (t.to(DEV) for t in IC.inputs(Q, R, K))
    stats = _stats(S, T, c)
    loss, d32, d16 = _loss(S, T, c, stats), _grad(S, T, c, stats, F32), _grad(S, T, c, stats, BF16)
    ref_loss, s_stats, t_stats = D._loss_forward(S, T, c, Q, Q, R, K, INV_TS, INV_TT)
    one = torch.ones((), dtype=torch.float32, device=DEV)
    ref32 = D._loss_grad(F32, S, T, c, Q, Q, R, K, INV_TS, INV_TT, s_stats, t_stats, one)
    ref16 = D._loss_grad(BF16, S, T, c, Q, Q, R, K, INV_TS, INV_TT, s_stats, t_stats, one)
    torch.cuda.synchronize()
    assert abs(float(loss) - float(ref_loss)) <= 1e-4 * abs(float(ref_loss))
    assert d32.shape == ref32.shape and d16.shape == ref16.shape
    _check_grads("vs dino_grad", d32.cpu().double().numpy(), d16.cpu().double().numpy(), ref32.cpu().double().numpy())
    # the two bf16 results round nearly equal f32 values: each within the bf16 bound of the other kernel's f32 result
    _check_grads("dino_grad vs ibot f32", ref32.cpu().double().numpy(), ref16.cpu().double().numpy(), d32.cpu().double().numpy())


def test_dloss_scales_the_gradient_exactly():
    (S, T, c), _ = _case((2, 257, 1000))
    stats = _stats(S, T, c)
    for dt in (F32, BF16):
        full, half = _grad(S, T, c, stats, dt, 1.0), _grad(S, T, c, stats, dt, 0.5)
        torch.cuda.synchronize()
        assert float(full.abs().max()) > 0 and torch.equal(half, 0.5 * full), dt


@pytest.mark.parametrize("what,Q,R,K,ldr", [("K % 4", 2, 8, 1002, 16), ("ldr", 2, 8, 1000, 15), ("views", 65, 8, 1000, 520), ("rows", 2, 32768, 1000, 65536),
                                             ("empty", 2, 0, 1000, 16)])
def test_c_abi_refuses_unsupported_shapes_and_writes_nothing(what, Q, R, K, ldr):
    lib = L.lib()
    f = lambda n: torch.full((n,), 7.0, dtype=torch.float32, device=DEV)      # noqa: E731
    S, T, c, st, loss, dST, one = f(64), f(64), f(1024), f(64), f(1), f(64), f(1)
    ws = torch.full((4096,), 0x5A, dtype=torch.uint8, device=DEV)
    if what != "ldr":
        rc = lib.m3l_op_ibot_loss(L.ptr(S), L.ptr(T), Q, R, K, L.ptr(c), INV_TS, INV_TT, L.ptr(st), L.ptr(st), L.ptr(ws), L.ptr(loss), _stream())
        assert rc != 0 and "ibot_loss" in L.last_error()
    rc = lib.m3l_op_ibot_grad(F32, L.ptr(S), L.ptr(T), Q, R, K, L.ptr(c), INV_TS, INV_TT, L.ptr(st), L.ptr(st), L.ptr(one), L.ptr(dST), ldr, _stream())
    assert rc != 0 and "ibot_grad" in L.last_error()
    if what in ("K % 4", "empty"):
        rc = lib.m3l_op_ibot_center_sum(L.ptr(T), Q * R, K, 1.0, L.ptr(ws), L.ptr(loss), _stream())
        assert rc != 0 and "ibot_center_sum" in L.last_error()
    torch.cuda.synchronize()
    assert all(bool((t == 7).all()) for t in (S, T, c, st, loss, dST, one)) and bool((ws == 0x5A).all())


def _module_run(mod, S, T, **kw):
    s = S.clone().requires_grad_(True)
    loss = mod(list(s.unbind(0)), T, TT, **kw)              # the student as a list of Q (R, K) tensors, the teacher as (Q, R, K)
    loss.backward()
    torch.cuda.synchronize()
    assert loss.dtype == torch.float32 and loss.dim() == 0
    return loss.detach(), s.grad


@pytest.mark.parametrize("shape", list(IC.RECORDED))
def test_module_against_the_recorded_cases_in_both_centering_modes(shape):
    (S, T, c), r, p_sk, r_sk = (_case(shape)[0],) + restated(shape)[1:]
    Q, R, K = shape
    n = IC.RECORDED[shape]
    gmax = float(np.abs(r["dS"]).max())
    # centred targets: the centre is used as it stands, this call's sums wait (one-step delay)
    mod = m3l_amd.iBOTPatchLoss(patch_out_dim=K).to(DEV)
    mod.center.copy_(c.view(1, 1, K))
    loss, grad = _module_run(mod, S, T)
    assert abs(float(loss) - r["loss"]) <= 1e-4 * abs(r["loss"])
    assert float(np.abs(grad.cpu().double().numpy() - r["dS"]).max()) <= 1e-4 * gmax
    assert mod.updated is False and torch.equal(mod.center.view(-1), c) and mod.len_teacher_patch_tokens == Q
    np.testing.assert_allclose(mod.async_batch_center.cpu().numpy().ravel(), r["pending"] * n / R, rtol=1e-5, atol=1e-5)
    mod.apply_center_update()
    np.testing.assert_allclose(mod.center.cpu().numpy().ravel(), r["center_after"], rtol=1e-5, atol=1e-5)
    assert mod.updated is True and tuple(mod.center.shape) == (1, 1, K)
    # the reference's call form: (Q B, n, K) teacher tokens
    mod.center.copy_(c.view(1, 1, K))
    probs = mod.softmax_center_teacher(T.view(Q * R // n, n, K), TT)
    mod.update_center(T.view(Q * R // n, n, K))
    assert probs.shape == (Q * R // n, n, K) and mod.len_teacher_patch_tokens == Q * R // n
    assert float(np.abs(probs.view(Q, R, K).cpu().double().numpy() - r["probs"]).max()) <= 1e-4 * float(r["probs"].max())
    np.testing.assert_allclose(mod.async_batch_center.cpu().numpy().ravel(), r["pending"], rtol=1e-5, atol=1e-5)
    # Sinkhorn-Knopp targets over all Q R rows: the pending update stays pending, the centre is untouched
    pending = mod.async_batch_center.clone()
    loss_sk, grad_sk = _module_run(mod, S, T, centering="sinkhorn_knopp")
    assert abs(float(loss_sk) - r_sk["loss"]) <= 1e-4 * abs(r_sk["loss"])
    assert float(np.abs(grad_sk.cpu().double().numpy() - r_sk["dS"]).max()) <= 1e-4 * float(np.abs(r_sk["dS"]).max())
    assert mod.updated is False and torch.equal(mod.center.view(-1), c) and torch.equal(mod.async_batch_center, pending)
    p = mod.sinkhorn_knopp_teacher(T.view(Q * R, K), TT, torch.tensor(n))
    p2 = mod.sinkhorn_knopp_teacher(T.view(Q * R, K), TT, torch.tensor(1000))
    torch.cuda.synchronize()
    assert torch.equal(p, p2) and p.shape == (Q * R, K)
    assert float(np.abs(p.view(Q, R, K).cpu().double().numpy() - p_sk).max()) <= 1e-4 * float(p_sk.max())
    with pytest.raises(ValueError, match="centering"):
        mod(S, T, TT, centering="none")


# ---- steps ---------------------------------------------------------------------------------------------------------------------------------
def _step_inputs():
    return {k: torch.from_numpy(_z(f"vtdino_ibot_step_inputs_{k}.npz")["input/" + k]).to(DEV) for k in ("image", "tactile1", "tactile2")}


def _step_model(dt="fp32", **kw):
    """The step fixture's module with its recorded parameters (the patch centre starts at zero, as the reference's)."""
    z = _z("vtdino_ibot_step.npz")
    model = build_step_module(z, compute_dtype=dt, allow_mask_overlap=True, **kw)
    sd = {k[len("param/"):]: torch.from_numpy(z[k]) for k in z.files if k.startswith("param/")}
    for k in list(sd):
        if k.startswith("student_encoder.backbone."):
            sd["teacher_encoder.backbone." + k[len("student_encoder.backbone."):]] = sd[k].clone()
    missing, unexpected = model.load_state_dict(sd, strict=False)
    assert not unexpected and all(k == "ibot_patch_loss.center" or ".ibot_head." in k for k in missing), (missing, unexpected)
    return model.to(DEV)


def _max_rel(got, ref):
    return float(np.abs(got - ref).max()) / max(1e-30, float(np.abs(ref).max()))


def _rel_l2(got, ref):
    return float(np.linalg.norm((got - ref).ravel())) / max(1e-30, float(np.linalg.norm(ref.ravel())))


@pytest.mark.parametrize("dt", ["fp32", "bf16"])
@pytest.mark.parametrize("centering", ["centering", "sinkhorn_knopp"])
def test_two_steps_against_the_reference_fixtures(centering, dt):
    """Two consecutive steps of VTDINO(ibot=True) (shared head, B = 8, 2 global views, R = 8 x 147 then 8 x 108 patch rows per view: above the old
    255 limit and no multiple of a tile) from the fixture's parameters: masks, total / DINO / patch losses, register logits, every student gradient,
    the patch centre's one-step delay.  fp32: loss 1e-4 relative, gradients 2e-3 of the largest entry; bf16: twice the recorded errors of the
    bf16-operand emulation.  Measured on an MI355X (step 1 / step 2; bound in brackets):
      centering       fp32  loss rel 6.1e-8 / 2.1e-7 (1e-4)  patch term 1.4e-7 / 1.5e-7 (1e-4)  grad max-rel 1.1e-6 / 3.2e-6 (2e-3)
                      bf16  loss rel 5.1e-4 / 2.4e-3 (1.0e-3 / 4.6e-3)  patch term 6.8e-4 / 2.1e-3 (1.4e-3 / 4.4e-3)
                            grad max-rel 1.1e-2 / 2.4e-2 (2.3e-2 / 4.6e-2)  rel-L2 9.2e-3 / 2.0e-2 (1.8e-2 / 3.7e-2)  logits 1.8e-3 / 4.5e-3 (3.7e-3 / 9.3e-3)
      sinkhorn_knopp  fp32  loss rel 1.8e-8 / 1.9e-9 (1e-4)  patch term 2.4e-8 / 1.3e-8 (1e-4)  grad max-rel 8.0e-7 / 1.1e-6 (2e-3)
                      bf16  loss rel 3.6e-4 / 5.0e-5 (7.4e-4 / 1.6e-4)  patch term 6.3e-5 / 2.9e-5 (1.3e-4 / 1.5e-4)
                            grad max-rel 2.8e-2 / 1.7e-2 (5.5e-2 / 3.1e-2)  rel-L2 1.5e-2 / 1.4e-2 (3.1e-2 / 2.6e-2)  logits 1.8e-3 / 4.4e-3 (3.7e-3 / 8.9e-3)"""
    stem = "vtdino_ibot_step" if centering == "centering" else "vtdino_ibot_sk_step"
    z, zp = _z(stem + ".npz"), _z("vtdino_ibot_step.npz")
    model = _step_model(dt, ibot=True, centering=centering)
    x = _step_inputs()
    lr, Q, B = float(zp["meta/lr"]), 2, 8
    pl = model.ibot_patch_loss
    for s in (1, 2):
        zs = _z(f"{stem}_s{s}.npz")
        for p in model.parameters():
            p.grad = None
        center_before = pl.center.clone()
        out = model.training_step(x, s - 1)
        out["loss"].backward()
        torch.cuda.synchronize()
        model.generator.manual_seed(s - 1)
        gm, _ = model.sample_masks(x["image"])
        assert all(np.array_equal(m.cpu().numpy(), zp[f"mask/{s - 1}/global/{i}"]) for i, m in enumerate(gm))
        n = int(z[f"step{s}/patches_per_view_row"])
        assert tuple(model.last["student_patch_logits"].shape) == (Q, B * n, int(zp["meta/K"])) == tuple(model.last["teacher_patch_logits"].shape)
        assert set(out) == {"ssl_loss", "dino_loss", "ibot_loss", "loss", "online_probes_loss"}
        assert all(isinstance(out[k], float) for k in ("ssl_loss", "dino_loss", "ibot_loss")) and float(out["loss"]) == out["ssl_loss"]
        assert abs(out["dino_loss"] + out["ibot_loss"] - out["ssl_loss"]) <= 1e-6 * abs(out["ssl_loss"])
        ref_loss, ref_dino, ref_ibot = (float(z[f"step{s}/{k}"]) for k in ("loss", "dino_loss", "ibot_loss"))
        loss_rel = abs(out["ssl_loss"] - ref_loss) / abs(ref_loss)
        ibot_rel = abs(out["ibot_loss"] - ref_ibot) / abs(ref_ibot)
        named = dict(model.student_encoder.named_parameters())
        grad_names = [k[len("grad/"):] for k in zs.files if k.startswith("grad/")]
        emax = {k: _max_rel(named[k].grad.cpu().numpy(), zs["grad/" + k]) for k in grad_names}
        el2 = {k: _rel_l2(named[k].grad.cpu().numpy(), zs["grad/" + k]) for k in grad_names}
        s_err = float(np.abs(model.last["student_logits"].cpu().numpy() - zs["student_logits"]).max())
        t_err = float(np.abs(model.last["teacher_logits"].cpu().numpy() - zs["teacher_logits"]).max())
        pre = f"bf16emu/step{s}/"
        if dt == "fp32":
            b_loss, b_ibot, b_max, b_l2 = 1e-4, 1e-4, 2e-3, None
            b_s = b_t = 1e-4 + 1e-3 * float(np.abs(zs["student_logits"]).max())
        else:
            b_loss, b_ibot = 2 * float(z[pre + "loss_rel"]), 2 * float(z[pre + "ibot_rel"])
            b_max, b_l2 = 2 * float(z[pre + "grad_max_rel"].max()), 2 * float(z[pre + "grad_rel_l2"].max())
            b_s, b_t = 2 * float(z[pre + "student_logits_max_abs"]), 2 * float(z[pre + "teacher_logits_max_abs"])
        worst = max(emax, key=emax.get)
        print(f"[{centering} {dt}] step {s}: loss {out['ssl_loss']:.6f} ref {ref_loss:.6f} rel {loss_rel:.3e} (bound {b_loss:.3e})  ibot {out['ibot_loss']:.6f} "
              f"ref {ref_ibot:.6f} rel {ibot_rel:.3e} (bound {b_ibot:.3e})  dino {out['dino_loss']:.6f} ref {ref_dino:.6f}  grad max-rel worst "
              f"{emax[worst]:.3e} at {worst} (bound {b_max:.3e})  rel-L2 worst {max(el2.values()):.3e} (bound {b_l2})  logits max-abs student {s_err:.3e} "
              f"(bound {b_s:.3e}) teacher {t_err:.3e} (bound {b_t:.3e})")
        assert loss_rel <= b_loss, (s, loss_rel, b_loss)
        assert ibot_rel <= b_ibot, (s, ibot_rel, b_ibot)
        assert s_err <= b_s and t_err <= b_t, (s, s_err, b_s, t_err, b_t)
        for k in grad_names:
            assert emax[k] <= b_max, (s, k, emax[k], b_max)
            if b_l2 is not None:
                assert el2[k] <= b_l2, (s, k, el2[k], b_l2)
        for u in z[f"step{s}/unused_params"]:
            assert named[str(u)].grad is None, u
        assert all(p.grad is None for p in model.teacher_encoder.parameters()), "the teacher received a gradient"
        if centering == "centering":
            # the centre this step used is the one the previous step left pending; this step's sums wait.  A pending entry is a sum of
            # Q B = 16 per-sample means of teacher logits, so 16 times the logits' bound holds for it
            used = torch.zeros_like(center_before) if s == 1 else MOM * center_before + (1 - MOM) * pending_prev / (Q * B)
            assert pl.updated is False and torch.allclose(pl.center, used, rtol=1e-6, atol=1e-9)
            assert float(np.abs(pl.center.cpu().numpy().ravel() - z[f"step{s}/ibot_center_used"]).max()) <= (1 - MOM) * b_t + 1e-7
            assert float(np.abs(pl.async_batch_center.cpu().numpy().ravel() - z[f"step{s}/ibot_pending"]).max()) <= Q * B * b_t
            pending_prev = pl.async_batch_center.clone().view(1, 1, -1)
        else:
            assert not pl.center.any() and pl.updated is True and pl.async_batch_center is None and not model.dino_loss.center.any()
        with torch.no_grad():
            for p in model.student_encoder.parameters():
                if p.grad is not None:
                    p.sub_(lr * p.grad)
        model.on_train_batch_end(out, x, s - 1)


def _one_step(model, x):
    out = model.training_step(x, 0)
    out["loss"].backward()
    torch.cuda.synchronize()
    return out, {k: p.grad.clone() for k, p in model.student_encoder.named_parameters() if p.grad is not None}


def test_ibot_false_is_the_step_without_the_keyword():
    x = _step_inputs()
    runs = [_one_step(_step_model(**kw), x) for kw in ({}, {"ibot": False, "ibot_separate_head": False})]
    (o0, g0), (o1, g1) = runs
    assert set(o0) == set(o1) == {"ssl_loss", "loss", "online_probes_loss"} and o0["ssl_loss"] == o1["ssl_loss"]
    assert g0.keys() == g1.keys() and all(torch.equal(g0[k], g1[k]) for k in g0)


@pytest.mark.parametrize("centering", ["centering", "sinkhorn_knopp"])
def test_three_terms_add_up_and_the_teacher_gets_no_gradient(centering):
    model = _step_model(ibot=True, koleo_weight=0.1, centering=centering)
    out, grads = _one_step(model, _step_inputs())
    assert set(out) == {"ssl_loss", "dino_loss", "ibot_loss", "koleo_loss", "loss", "online_probes_loss"}
    assert abs(out["dino_loss"] + out["ibot_loss"] + out["koleo_loss"] - out["ssl_loss"]) <= 1e-6 * abs(out["ssl_loss"])
    assert out["ibot_loss"] > 0 and all(np.isfinite(out[k]) for k in ("ssl_loss", "dino_loss", "ibot_loss", "koleo_loss"))
    assert all(p.grad is None for p in model.teacher_encoder.parameters()) and all(bool(torch.isfinite(g).all()) for g in grads.values())
    # the same step without the two extra terms: the DINO term is the same number
    plain, _ = _one_step(_step_model(centering=centering), _step_inputs())
    assert abs(plain["ssl_loss"] - out["dino_loss"]) <= 1e-6 * abs(plain["ssl_loss"])


def test_separate_head_leaves_the_dino_prototype_gradient_to_the_dino_term():
    x = _step_inputs()
    plain = _step_model()
    torch.manual_seed(11)
    sep = _step_model(ibot=True, ibot_separate_head=True)
    _, g_plain = _one_step(plain, x)
    out, g_sep = _one_step(sep, x)
    for k in ("dino_head.last_layer.weight_v", "dino_head.last_layer.weight_g"):
        assert torch.equal(g_plain[k], g_sep[k]), k
    for k, p in sep.student_encoder["ibot_head"].named_parameters():
        assert p.grad is not None and float(p.grad.abs().max()) > 0, k
    assert not any(k.startswith("ibot_head.") for k in g_plain) and out["ibot_loss"] > 0
    # shared head: the patch rows do reach dino_head's prototypes
    _, g_shared = _one_step(_step_model(ibot=True), x)
    assert not torch.equal(g_plain["dino_head.last_layer.weight_v"], g_shared["dino_head.last_layer.weight_v"])


@pytest.mark.parametrize("dt", ["fp32", "bf16"])
def test_prototype_layer_backward_in_row_chunks_equals_one_call(monkeypatch, dt):
    """dx_n = dS W reduces over the K prototypes; past 2 GiB per operand (f32: 65536 prototypes x more than 8191 rows) it runs in chunks of
    prototype rows that accumulate.  Here the limit is lowered so that K = 1000 takes 8 chunks: the same gradients as the single call, up to the
    order of the f32 sums (1e-5 of the largest entry), and the same bits on a second run."""
    (S, T, c), _ = _case((2, 257, 1000))
    Q, R, K = S.shape
    g = torch.Generator().manual_seed(5)
    xn0 = torch.nn.functional.normalize(torch.randn(Q * R, 32, generator=g), dim=-1).to(DEV)
    v0, g0 = torch.randn(K, 32, generator=g).to(DEV), (0.5 + torch.rand(K, 1, generator=g)).to(DEV)

    def run():
        xn, v, gg = (t.clone().requires_grad_(True) for t in (xn0, v0, g0))
        loss = D.IbotHeadLossFn.apply(F32 if dt == "fp32" else BF16, Q, xn, v, gg, T, c, TS, TT, None)
        loss.backward()
        torch.cuda.synchronize()
        return loss.detach(), xn.grad, v.grad, gg.grad
    whole = run()
    esize, ldr = (4 if dt == "fp32" else 2), D._ld8(Q * R)
    monkeypatch.setattr(D, "TN_OPERAND_LIMIT", 128 * ldr * esize + 1)           # chunks of 128 prototype rows
    calls = []
    real = L.lib().m3l_op_gemm_tn_acc
    monkeypatch.setattr(L.lib(), "m3l_op_gemm_tn_acc", lambda *a: calls.append(a[-2]) or real(*a))
    cut, again = run(), run()
    assert calls == ([0] + [1] * 7) * 2, calls
    assert torch.equal(whole[0], cut[0]) and torch.equal(whole[2], cut[2]) and torch.equal(whole[3], cut[3])      # only dx_n takes the TN GEMM
    assert float((whole[1] - cut[1]).abs().max()) <= 1e-5 * float(whole[1].abs().max())
    assert all(torch.equal(a, b) for a, b in zip(cut, again)), "two runs differ in their bits"


@pytest.mark.parametrize("dt", ["bf16", "fp32"])
def test_full_size_step_completes_and_repeats_bit_for_bit(dt):
    """B = 32, 2 + 8 views, K = 65536, the reference configuration's encoder and head: not a parity check.  In fp32 dS^T is 65536 x 9408 floats,
    past the 2 GiB an operand of the TN GEMM may have, so dx_n takes the chunked route for real."""
    g = torch.Generator().manual_seed(1)
    x = {"image": torch.rand(32, 3, 64, 64, generator=g).to(DEV), "tactile1": torch.rand(32, 3, 32, 32, generator=g).to(DEV),
         "tactile2": torch.rand(32, 3, 32, 32, generator=g).to(DEV)}
    torch.manual_seed(0)
    enc = m3l_amd.DinoVTT(image_size=64, tactile_size=32, image_patch_size=8, tactile_patch_size=4, dim=256, depth=4, heads=8, mlp_dim=512,
                          num_tactiles=2, num_register_tokens=1, compute_dtype=dt)
    model = m3l_amd.VTDINO(encoder=enc, dino_head=partial(m3l_amd.DINOHead, out_dim=65536, nlayers=3, hidden_dim=2048, bottleneck_dim=256),
                           optim_cfg=None, lr_scheduler_cfg=None, wd_scheduler_cfg=None, local_mask_scale=(0.2, 0.48), global_mask_scale=(0.48, 1.0),
                           num_global_masks=2, num_local_masks=8, allow_mask_overlap=True, teacher_temp=0.05, ibot=True, koleo_weight=0.1).to(DEV)
    model.current_teacher_temp = 0.05
    runs = []
    for _ in range(2):
        for p in model.parameters():
            p.grad = None
        model.step = -1
        model.ibot_patch_loss.updated = model.dino_loss.updated = True      # both runs start from the same (zero) centres
        out = model.training_step(x, 0)
        out["loss"].backward()
        torch.cuda.synchronize()
        runs.append((out["ssl_loss"], out["ibot_loss"], {k: p.grad.clone() for k, p in model.student_encoder.named_parameters() if p.grad is not None}))
    Q, R, K = model.last["student_patch_logits"].shape
    print(f"full size: Q = {Q}, R = {R} patch rows per view, K = {K}, loss {runs[0][0]:.4f}, ibot {runs[0][1]:.4f}")
    assert (Q, K) == (2, 65536) and R % 32 == 0 and R >= 32 * 3 * 25 and np.isfinite(runs[0][0])
    assert runs[0][:2] == runs[1][:2] and all(torch.equal(runs[0][2][k], runs[1][2][k]) for k in runs[0][2])
    # values at this size (2.47 GB per logit tensor: a 32-bit offset would wrap): the patch term against torch in float64 over all rows of the stored
    # logits (zero centre: the first step), and the last eight pair-rows of the gradient kernel's output, the highest addresses it touches
    S, T = model.last["student_patch_logits"], model.last["teacher_patch_logits"]
    ts, tt = model.ibot_patch_loss.student_temp, model.current_teacher_temp
    total = torch.zeros((), dtype=torch.float64, device=DEV)
    for r0 in range(0, R, 294):
        lsm = torch.log_softmax(S[:, r0:r0 + 294].double() / ts, dim=-1)
        p = torch.softmax(T[:, r0:r0 + 294].double() / tt, dim=-1)
        total -= (p.sum(0, keepdim=True) * lsm).sum()
    ref = float(total) / R / Q
    assert abs(runs[0][1] - ref) <= 1e-4 * abs(ref), (runs[0][1], ref)
    c0 = torch.zeros(K, dtype=torch.float32, device=DEV)
    s_stats, t_stats = D._row_stats(S, Q * R, K, None, 1.0 / ts), D._row_stats(T, Q * R, K, c0, 1.0 / tt)
    one = torch.ones((), dtype=torch.float32, device=DEV)
    dST = D._ibot_grad(F32, S, T, c0, Q, R, K, 1.0 / ts, 1.0 / tt, s_stats, t_stats, one)
    got = dST[:, Q * R - 8:Q * R].t().double()
    want = (Q * torch.softmax(S[-1, -8:].double() / ts, dim=-1) - torch.softmax(T[:, -8:].double() / tt, dim=-1).sum(0)) / (ts * R)
    err = float((got - want).abs().max() / want.abs().max())
    print(f"full size {dt}: patch term {runs[0][1]:.6f} torch float64 {ref:.6f}; last rows of dS^T err {err:.2e} of the largest entry")
    assert err <= 1e-4, err


# ---- memory contract -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(2, 257, 1000), (2, 35, 65536)])
def test_memory_contract_of_the_ops(monkeypatch, shape):
    (S, T, c), _ = _case(shape)
    Q, R, K = shape

    def work(g):
        mod = m3l_amd.iBOTPatchLoss(patch_out_dim=K).to(DEV)
        mod.center.copy_(c.view(1, 1, K))
        s = S.clone().requires_grad_(True)
        loss = mod(s, T, TT)                                 # row statistics, m3l_op_ibot_loss, m3l_op_ibot_center_sum
        g.check("after the forward")
        loss.backward()                                      # m3l_op_ibot_grad, f32
        g.check("after the backward")
        s_stats, t_stats = _stats(S, T, c)
        one = torch.ones((), dtype=torch.float32, device=DEV)
        d16 = D._ibot_grad(BF16, S, T, c, Q, R, K, INV_TS, INV_TT, s_stats, t_stats, one)
        g.check("after the bf16 gradient")
        return {"loss": loss, "grad": s.grad, "pending": mod.async_batch_center, "d16": d16}
    counts = MG.run_contract(monkeypatch, work)
    assert counts[0] == counts[1] and counts[0][0] >= 4


def test_memory_contract_of_a_step_with_the_patch_loss(monkeypatch):
    g0 = torch.Generator().manual_seed(100)
    x = {k: torch.rand(4, 3, 32, 32, generator=g0).to(DEV) for k in ("image", "tactile1", "tactile2")}

    def work(g):
        torch.manual_seed(0)
        enc = m3l_amd.DinoVTT(image_size=32, tactile_size=32, image_patch_size=8, tactile_patch_size=8, dim=64, depth=2, heads=2, mlp_dim=128,
                              num_tactiles=2, num_register_tokens=1)
        model = m3l_amd.VTDINO(encoder=enc, dino_head=partial(m3l_amd.DINOHead, out_dim=512, hidden_dim=64, bottleneck_dim=32), optim_cfg=None,
                               lr_scheduler_cfg=None, wd_scheduler_cfg=None, local_mask_scale=(0.45, 0.6), global_mask_scale=(0.7, 1.0),
                               num_global_masks=2, num_local_masks=3, allow_mask_overlap=True, teacher_temp=0.05, ibot=True).to(DEV)
        model.current_teacher_temp = 0.05
        out = model.training_step(x, 0)
        g.check("after the forward")
        out["loss"].backward()
        g.check("after the backward")
        grads = {k: p.grad for k, p in model.student_encoder.named_parameters() if p.grad is not None}
        return {"loss": out["loss"], "ibot": out["ibot_loss"], "pending": model.ibot_patch_loss.async_batch_center, "grad": grads}
    MG.run_contract(monkeypatch, work)
