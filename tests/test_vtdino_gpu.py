"""GPU checks of the DINO self-distillation stack: the new kernels through the C ABI against float64, the module against the two-step
fixture recorded from the reference's classes (tests/golden/make_golden_vtdino.py), and one full-size run of the reference configuration.

Yardsticks.  Kernels: torch float64 on the same inputs; for the loss, `dino_loss_restated` below — a plain float64 restatement of the
reference loss in its own pairwise form — which `test_restatement_equals_reference_fixture` (CPU) pins to dino_loss_f64.npz, the
reference DINOLoss's recorded float64 results.  Module: the float64 run of the reference stored in vtdino_step*.npz.

Bounds.  fp32 mode (exact f32 MFMA): the project's fp32 bounds — loss 1e-4 relative, every gradient within 2e-3 of its largest entry
(tests/test_parity_gpu.py).  Loss kernels on their own: loss 1e-4 relative; dS and the row statistics 1e-4 of the largest entry — the
scaled logits reach |z| ~ 200, so z carries 200 * 2^-24 ~ 1e-5 of absolute rounding into exp(), a relative 1e-5 per element, and
v_exp_f32 adds about as much; 1e-4 leaves a factor 5.  bf16 storage of dS / W: one rounding, 2^-8 relative.  bf16 mode of the module:
nothing is assumed; the fixture records the error of a float32 run of the reference with every matrix product's operands rounded to
bf16 (forward and backward) against the float64 run, and the bound is twice the largest recorded value of the step (the factor covers
accumulation order and the bf16 kernels' fitted GELU, which the emulation does not reproduce; the largest value over the parameters,
because a single tensor's recorded error depends on the rounding pattern it happened to meet).
"""
import ctypes as C
import os
from functools import partial

import numpy as np
import pytest
import torch

import m3l_amd
from m3l_amd import _lib as L
from m3l_amd import dino as D
from test_vtdino_cpu import _z, build_step_module, load_step_params

gpu = pytest.mark.gpu
DEV = "cuda:0"


def _stream():
    return torch.cuda.current_stream().cuda_stream


def dino_loss_restated(S, T, center, student_temp, teacher_temp):
    """float64, pairwise: sum_p sum_q mean_b( -sum_k softmax((T[q] - center) / tt) * log_softmax(S[p] / ts) ).  -> loss, probs"""
    probs = torch.softmax((T - center) / teacher_temp, dim=-1)
    total = 0
    for p in range(S.shape[0]):
        lsm = torch.log_softmax(S[p] / student_temp, dim=-1)
        for q in range(T.shape[0]):
            total = total - torch.sum(probs[q] * lsm, dim=-1).mean()
    return total, probs


def test_restatement_equals_reference_fixture():
    z = _z("dino_loss_f64.npz")
    for call in range(2):
        pre = f"call{call}/"
        S = torch.from_numpy(z[pre + "S"]).requires_grad_(True)
        loss, probs = dino_loss_restated(S, torch.from_numpy(z[pre + "T"]), torch.from_numpy(z[pre + "center_used"]), float(z["student_temp"]),
                                         float(z[pre + "teacher_temp"]))
        loss.backward()
        assert abs(float(loss) - float(z[pre + "loss"])) <= 1e-12 * abs(float(z[pre + "loss"]))
        assert np.abs(probs.numpy() - z[pre + "probs"]).max() <= 1e-14
        assert np.abs(S.grad.numpy() - z[pre + "dS"]).max() <= 1e-13


# ---- kernels -------------------------------------------------------------------------------------------------------------------------
@gpu
def test_l2norm_fwd_bwd_against_float64():
    g = torch.Generator().manual_seed(0)
    M, Dm, eps = 37, 100, 1e-12
    x = torch.randn(M, Dm, generator=g)
    x[5] = 0.0                                   # clamped row: y = 0, dx = dy / eps
    dy = torch.randn(M, Dm, generator=g)
    xd = x.double().requires_grad_(True)
    yd = torch.nn.functional.normalize(xd, dim=-1, p=2, eps=eps)
    yd.backward(dy.double())
    xg, dyg = x.to(DEV), dy.to(DEV)
    y32 = torch.empty_like(xg)
    yb = torch.empty(M, Dm, dtype=torch.bfloat16, device=DEV)
    norm = torch.empty(M, device=DEV)
    L.check(L.lib().m3l_op_l2norm_fwd(1, L.ptr(xg), M, Dm, eps, L.ptr(yb), L.ptr(y32), L.ptr(norm), _stream()), "l2norm_fwd")
    dx = torch.empty_like(xg)
    L.check(L.lib().m3l_op_l2norm_bwd(L.ptr(dyg), L.ptr(xg), L.ptr(norm), M, Dm, eps, L.ptr(dx), _stream()), "l2norm_bwd")
    assert (y32.cpu().double() - yd.detach()).abs().max() <= 1e-6
    assert (yb.cpu().double() - yd.detach()).abs().max() <= 2.0 ** -8
    assert (norm.cpu().double() - x.double().norm(dim=-1)).abs().max() <= 1e-5
    ref = xd.grad
    rows = torch.arange(M) != 5
    assert (dx.cpu().double()[rows] - ref[rows]).abs().max() <= 1e-5 * ref[rows].abs().max()
    assert (dx.cpu().double()[5] - ref[5]).abs().max() <= 1e-6 * ref[5].abs().max()


@gpu
@pytest.mark.parametrize("dt", [0, 1])
def test_weightnorm_fwd_bwd_against_float64(dt):
    g = torch.Generator().manual_seed(1)
    K, Dm = 130, 40
    v = torch.randn(K, Dm, generator=g)
    gg = torch.rand(K, 1, generator=g) + 0.5
    dW = torch.randn(K, Dm, generator=g)
    vd, gd = v.double().requires_grad_(True), gg.double().requires_grad_(True)
    Wd = torch._weight_norm(vd, gd, 0)
    Wd.backward(dW.double())
    tdt = torch.bfloat16 if dt else torch.float32
    vg, ggpu, dWg = v.to(DEV), gg.to(DEV), dW.to(DEV)
    W = torch.empty(K, Dm, dtype=tdt, device=DEV)
    vnorm = torch.empty(K, device=DEV)
    L.check(L.lib().m3l_op_weightnorm_fwd(dt, L.ptr(vg), L.ptr(ggpu), K, Dm, L.ptr(W), L.ptr(vnorm), _stream()), "weightnorm_fwd")
    tol = 2.0 ** -8 if dt else 1e-6
    ref = Wd.detach()
    assert ((W.cpu().double() - ref).abs() <= tol * ref.abs() + 1e-7).all()
    assert (vnorm.cpu().double() - v.double().norm(dim=1)).abs().max() <= 1e-5
    dv, dg = torch.empty_like(vg), torch.empty_like(ggpu)
    L.check(L.lib().m3l_op_weightnorm_bwd(L.ptr(dWg), L.ptr(vg), L.ptr(ggpu), L.ptr(vnorm), K, Dm, L.ptr(dv), L.ptr(dg), _stream()), "weightnorm_bwd")
    assert (dv.cpu().double() - vd.grad).abs().max() <= 1e-5 * vd.grad.abs().max()
    assert (dg.cpu().double() - gd.grad).abs().max() <= 1e-5 * gd.grad.abs().max()


def _run_loss_kernels(S, T, center, ts, tt, dt=0, dloss=1.0):
    """S (P, B, K), T (Q, B, K), center (K) float32 on the GPU -> loss, dS, student stats, teacher stats."""
    (P, B, K), Q = S.shape, T.shape[0]
    loss, s_stats, t_stats = D._loss_forward(S, T, center, P, Q, B, K, 1.0 / ts, 1.0 / tt)
    dST = D._loss_grad(dt, S, T, center, P, Q, B, K, 1.0 / ts, 1.0 / tt, s_stats, t_stats, torch.tensor(dloss, device=S.device))
    ldr = (P * B + 7) // 8 * 8
    assert tuple(dST.shape) == (K, ldr) and float(dST[:, P * B:].float().abs().sum()) == 0.0      # k-major, pad columns zero
    return loss, dST.t()[:P * B].reshape(P, B, K), s_stats, t_stats


def _check_loss_kernels(S64, T64, c64, ts, tt, dloss=1.0):
    S64 = S64.clone().requires_grad_(True)
    ref, _ = dino_loss_restated(S64, T64, c64, ts, tt)
    (ref * dloss).backward()
    S, T, c = S64.detach().float().to(DEV), T64.float().to(DEV), c64.reshape(-1).float().to(DEV)
    loss, dS, s_stats, t_stats = _run_loss_kernels(S, T, c, ts, tt, 0, dloss)
    loss2, dS2, _, _ = _run_loss_kernels(S, T, c, ts, tt, 0, dloss)
    rel = abs(float(loss) - float(ref)) / abs(float(ref))
    gmax = float(S64.grad.abs().max())
    gerr = float((dS.cpu().double() - S64.grad).abs().max()) / gmax
    lse_s = torch.logsumexp(S64.detach() / ts, dim=-1).reshape(-1)
    lse_t = torch.logsumexp((T64 - c64) / tt, dim=-1).reshape(-1)
    serr = float((s_stats[:, 1].cpu().double() - lse_s).abs().max() / lse_s.abs().max().clamp_min(1.0))
    terr = float((t_stats[:, 1].cpu().double() - lse_t).abs().max() / lse_t.abs().max().clamp_min(1.0))
    mx_s = (S64.detach() / ts).amax(dim=-1).reshape(-1)
    print(f"dino loss kernels P={S.shape[0]} Q={T.shape[0]} B={S.shape[1]} K={S.shape[2]}: loss rel {rel:.2e}  dS {gerr:.2e} of max  "
          f"lse student {serr:.2e} teacher {terr:.2e}")
    assert rel <= 1e-4 and gerr <= 1e-4 and serr <= 1e-4 and terr <= 1e-4
    assert (s_stats[:, 0].cpu().double() - mx_s).abs().max() <= 1e-4 * mx_s.abs().max()
    assert torch.equal(loss, loss2) and torch.equal(dS, dS2), "two runs on the same input differ"
    dSb = _run_loss_kernels(S, T, c, ts, tt, 1, dloss)[1]
    assert dSb.dtype == torch.bfloat16
    assert ((dSb.cpu().double() - S64.grad).abs() <= 2.0 ** -8 * S64.grad.abs() + 2e-4 * gmax).all()
    return loss


@gpu
def test_loss_kernels_against_reference_fixture_k1000():
    """K = 1000 (no multiple of a 1024-column sweep), 9 student and 6 teacher rows (no multiple of a wave or a block), Q = 2, non-zero
    centre, both recorded calls; plus the centre kernels with the one-step delay."""
    z = _z("dino_loss_f64.npz")
    ts, m = float(z["student_temp"]), float(z["center_momentum"])
    center = torch.from_numpy(z["center0"]).float().to(DEV).contiguous()
    for call in range(2):
        pre = f"call{call}/"
        tt = float(z[pre + "teacher_temp"])
        assert np.abs(center.cpu().numpy() - z[pre + "center_used"]).max() <= 1e-6
        S64, T64, c64 = torch.from_numpy(z[pre + "S"]), torch.from_numpy(z[pre + "T"]), torch.from_numpy(z[pre + "center_used"])
        loss = _check_loss_kernels(S64, T64, c64, ts, tt, dloss=1.0 if call == 0 else 0.37)
        if call == 0:
            assert abs(float(loss) - float(z[pre + "loss"])) <= 1e-4 * abs(float(z[pre + "loss"]))
        Q, B, K = T64.shape
        T = T64.float().to(DEV)
        pending = torch.empty(1, K, device=DEV)
        L.check(L.lib().m3l_op_dino_center_sum(L.ptr(T), Q * B, K, L.ptr(pending), _stream()), "center_sum")
        np.testing.assert_allclose(pending.cpu().numpy(), z[pre + "pending"], rtol=1e-5, atol=1e-5)
        # what the NEXT call starts with
        L.check(L.lib().m3l_op_dino_center_apply(L.ptr(center), L.ptr(pending), K, m, 1 - m, float(Q * B), _stream()), "center_apply")
    np.testing.assert_allclose(center.cpu().numpy(), z["center_final"], rtol=1e-5, atol=1e-6)


@gpu
@pytest.mark.parametrize("P,Q,B,K", [(5, 2, 5, 4096), (10, 2, 32, 65536)])
def test_loss_kernels_against_restatement_large_k(P, Q, B, K):
    g = torch.Generator().manual_seed(K)
    S64 = (1.5 * torch.randn(P, B, K, generator=g)).double()
    T64 = (1.5 * torch.randn(Q, B, K, generator=g)).double()
    c64 = (0.2 * torch.randn(1, K, generator=g)).double()
    _check_loss_kernels(S64, T64, c64, 0.1, 0.04, dloss=1.0)


@gpu
def test_multi_tensor_ema_against_per_tensor_formula():
    g = torch.Generator().manual_seed(3)
    lens = [1, 3, 5, 4096, 4097, 5001, 12289] + [7 + i for i in range(130)]        # odd lengths, a length-1 tensor, more than one launch's table
    beta = 0.996
    dst = [torch.randn(n, generator=g).to(DEV) for n in lens]
    src = [torch.randn(n, generator=g).to(DEV) for n in lens]
    buf_d, buf_s = torch.randn(1030, generator=g).to(DEV), torch.randn(1030, generator=g).to(DEV)
    before = buf_d.clone()
    dst.append(buf_d[1:1027])                   # a view that is not 16-byte aligned
    src.append(buf_s[3:1029])
    want = [d * beta + (1.0 - beta) * s for d, s in zip(dst, src)]
    n = len(dst)
    arr_len = (C.c_long * n)(*[t.numel() for t in dst])
    L.check(L.lib().m3l_op_ema(L.ptr_array(dst), L.ptr_array(src), arr_len, n, beta, 1.0 - beta, _stream()), "m3l_op_ema")
    for i, (d, w) in enumerate(zip(dst, want)):
        assert torch.equal(d, w), (i, d.numel(), float((d - w).abs().max()))
    assert torch.equal(buf_d[:1], before[:1]) and torch.equal(buf_d[1027:], before[1027:]), "the launch wrote outside a tensor"


@gpu
def test_head_forward_backward_against_fixture():
    z = _z("dino_head_init.npz")
    in_dim, out_dim, hidden, bott = [int(v) for v in z["cfg"]]
    head = m3l_amd.DINOHead(in_dim, out_dim, hidden_dim=hidden, bottleneck_dim=bott)
    head.load_state_dict({k[len("param/"):]: torch.from_numpy(z[k]) for k in z.files if k.startswith("param/")}, strict=True)
    head = head.to(DEV)
    x = torch.from_numpy(z["x"]).to(DEV).requires_grad_(True)
    y = head(x)
    y.backward(torch.from_numpy(z["dy"]).to(DEV))
    np.testing.assert_allclose(y.detach().cpu().numpy(), z["y"], rtol=1e-3, atol=1e-5)
    for name, got in [("dx", x.grad)] + [("grad/" + n, p.grad) for n, p in head.named_parameters()]:
        ref = z[name]
        err = float(np.abs(got.cpu().numpy() - ref).max()) / max(1e-12, float(np.abs(ref).max()))
        assert err <= 2e-3, (name, err)


# ---- module --------------------------------------------------------------------------------------------------------------------------
def _max_rel(got, ref):
    return float(np.abs(got - ref).max()) / max(1e-30, float(np.abs(ref).max()))


def _rel_l2(got, ref):
    return float(np.linalg.norm((got - ref).ravel())) / max(1e-30, float(np.linalg.norm(ref.ravel())))


@gpu
@pytest.mark.parametrize("dt", ["fp32", "bf16"])
def test_two_steps_against_reference_fixture(dt):
    """Two consecutive steps from the fixture's parameters (the second runs with the centre left pending by the first): loss, logits, every
    student gradient, centre, pending sums and the teacher after on_train_batch_end.
    Measured on an MI355X (worst parameter; bound in brackets; for bf16 the bound is twice the recorded emulation error):
      fp32  step 1: loss rel 8.1e-08 (1e-4)  grad max-rel 3.2e-06 (2e-3)      step 2: loss rel 3.1e-07  grad max-rel 1.5e-05
      bf16  step 1: loss rel 4.2e-04 (8.2e-04)  grad max-rel 2.1e-02 (3.6e-02)  rel-L2 1.4e-02 (2.5e-02)  logits 2.1e-03 (4.1e-03)
            step 2: loss rel 2.1e-03 (4.1e-03)  grad max-rel 8.2e-02 (1.4e-01)  rel-L2 5.2e-02 (8.9e-02)  logits 6.3e-03 (1.0e-02)"""
    z = _z("vtdino_step.npz")
    model = build_step_module(z, compute_dtype=dt)
    load_step_params(model, z)
    model = model.to(DEV)
    x = {k: torch.from_numpy(z["input/" + k]).to(DEV) for k in ("image", "tactile1", "tactile2")}
    lr = float(z["meta/lr"])
    drift = {}
    for s in (1, 2):
        zs, zt = _z(f"vtdino_step_s{s}.npz"), _z(f"vtdino_teacher_s{s}.npz")
        for p in model.parameters():
            p.grad = None
        out = model.training_step(x, s - 1)
        out["loss"].backward()
        torch.cuda.synchronize()
        ref_loss = float(z[f"step{s}/loss"])
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
            b_loss, b_max, b_l2 = 2 * float(z[pre + "loss_rel"]), 2 * float(z[pre + "grad_max_rel"].max()), 2 * float(z[pre + "grad_rel_l2"].max())
            b_s, b_t = 2 * float(z[pre + "student_logits_max_abs"]), 2 * float(z[pre + "teacher_logits_max_abs"])
        worst = max(emax, key=emax.get)
        print(f"[{dt}] step {s}: loss {out['ssl_loss']:.6f} ref {ref_loss:.6f} rel {loss_rel:.3e} (bound {b_loss:.3e})  grad max-rel worst "
              f"{emax[worst]:.3e} at {worst} (bound {b_max:.3e})  rel-L2 worst {max(el2.values()):.3e} (bound {b_l2})  logits max-abs student "
              f"{s_err:.3e} (bound {b_s:.3e}) teacher {t_err:.3e} (bound {b_t:.3e})")
        assert loss_rel <= b_loss, (s, loss_rel, b_loss)
        assert s_err <= b_s and t_err <= b_t, (s, s_err, b_s, t_err, b_t)
        for n in grad_names:
            assert emax[n] <= b_max, (s, n, emax[n], b_max)
            if b_l2 is not None:
                assert el2[n] <= b_l2, (s, n, el2[n], b_l2)
        for u in z[f"step{s}/unused_params"]:
            assert named[str(u)].grad is None, u
        assert all(p.grad is None for p in model.teacher_encoder.parameters()), "the teacher received a gradient"
        with torch.no_grad():
            for p in model.student_encoder.parameters():
                if p.grad is not None:
                    p.sub_(lr * p.grad)
        model.on_train_batch_end(out, x, s - 1)
        # centre: one step late (zero after the first step), pending = this step's teacher column sums
        tol = dict(rtol=1e-4, atol=1e-5) if dt == "fp32" else dict(rtol=0, atol=b_t * int(z["meta/B"]) * int(z["meta/n_global"]))
        np.testing.assert_allclose(model.dino_loss.center.cpu().numpy(), z[f"step{s}/center"].reshape(1, -1), **tol)
        np.testing.assert_allclose(model.dino_loss.async_batch_center.cpu().numpy(), z[f"step{s}/pending"].reshape(1, -1), **tol)
        if s == 1:
            assert float(model.dino_loss.center.abs().max()) == 0.0
        teacher = dict(model.teacher_encoder.named_parameters())
        for k in zt.files:
            got, ref = teacher[k[len("teacher/"):]].detach().cpu().numpy(), zt[k]
            if dt == "fp32":
                np.testing.assert_allclose(got, ref, rtol=2e-3, atol=2e-5, err_msg=k)
            else:
                # teacher_s = d teacher_(s-1) + (1 - d) (student - lr (g_1 + .. + g_s)): each step's gradient error enters with a weight
                # below (1 - d) (1 + d) < 2 (1 - d), and a gradient's error is at most b_max of its largest entry
                n = k[len("teacher/"):]
                if "grad/" + n in zs.files:
                    drift[n] = drift.get(n, 0.0) + b_max * float(np.abs(zs["grad/" + n]).max())
                bound = 2 * (1 - float(z["meta/decay"])) * lr * drift.get(n, 0.0)
                assert float(np.abs(got - ref).max()) <= bound + 1e-6 * max(1.0, float(np.abs(ref).max())), (k, bound)


def _small_module(seed=0, **enc_kw):
    torch.manual_seed(seed)
    kw = dict(image_size=32, tactile_size=32, image_patch_size=8, tactile_patch_size=8, dim=64, depth=2, heads=2, mlp_dim=128, num_tactiles=2,
              num_register_tokens=1)
    kw.update(enc_kw)
    enc = m3l_amd.DinoVTT(**kw)
    model = m3l_amd.VTDINO(encoder=enc, dino_head=partial(m3l_amd.DINOHead, out_dim=512, hidden_dim=64, bottleneck_dim=32), optim_cfg=None,
                           lr_scheduler_cfg=None, wd_scheduler_cfg=None, local_mask_scale=(0.45, 0.6), global_mask_scale=(0.7, 1.0),
                           num_global_masks=2, num_local_masks=3, allow_mask_overlap=True, teacher_temp=0.05).to(DEV)
    model.current_teacher_temp = 0.05
    g = torch.Generator().manual_seed(seed + 100)
    x = {k: torch.rand(4, 3, 32, 32, generator=g).to(DEV) for k in ("image", "tactile1", "tactile2")}
    return model, x


@gpu
def test_same_step_counter_gives_same_masks_and_loss_and_teacher_gets_no_gradient():
    a, x = _small_module()
    b, _ = _small_module()
    seen = []
    for m in (a, b):
        real = m.sample_masks
        m.sample_masks = lambda t, real=real: seen.append(real(t)) or seen[-1]
        out = m.training_step(x, 0)
        out["loss"].backward()
        seen.append(out["ssl_loss"])
    (gm_a, lm_a), loss_a, (gm_b, lm_b), loss_b = seen
    assert loss_a == loss_b and np.isfinite(loss_a)
    assert all(torch.equal(p, q) for p, q in zip(gm_a + lm_a, gm_b + lm_b))
    assert all(p.grad is None for p in a.teacher_encoder.parameters())
    used = [n for n, p in a.student_encoder.named_parameters() if p.grad is not None]
    assert "dino_head.last_layer.weight_g" in used and "dino_head.last_layer.weight_v" in used and "backbone.register_tokens" in used
    for (n, p), (_, q) in zip(a.student_encoder.named_parameters(), b.student_encoder.named_parameters()):
        assert (p.grad is None) == (q.grad is None) and (p.grad is None or torch.equal(p.grad, q.grad)), n


@gpu
@pytest.mark.parametrize("enc_kw", [dict(dim_head=32), dict(dim_head=128, heads=1), dict(dropout=0.1)])
def test_step_runs_with_other_head_widths_and_dropout(enc_kw):
    model, x = _small_module(seed=1, **enc_kw)
    out = model.training_step(x, 0)
    out["loss"].backward()
    assert np.isfinite(out["ssl_loss"])
    for n, p in model.student_encoder.named_parameters():
        assert p.grad is None or torch.isfinite(p.grad).all(), n
    model.on_train_batch_end(out, x, 0)
    assert all(torch.isfinite(p).all() for p in model.teacher_encoder.parameters())


def _full_size_step(dt):
    torch.manual_seed(0)
    enc = m3l_amd.DinoVTT(image_size=64, tactile_size=32, image_patch_size=8, tactile_patch_size=4, dim=256, depth=4, heads=8, mlp_dim=512,
                          num_tactiles=2, num_register_tokens=1, compute_dtype=dt)
    model = m3l_amd.VTDINO(encoder=enc, dino_head=partial(m3l_amd.DINOHead, out_dim=65536, use_bn=False, nlayers=3, hidden_dim=2048, bottleneck_dim=256),
                           optim_cfg=None, lr_scheduler_cfg=None, wd_scheduler_cfg=None, local_mask_scale=(0.2, 0.48), global_mask_scale=(0.48, 1.0),
                           num_global_masks=2, num_local_masks=8, min_keep_num_sensors=4, allow_mask_overlap=True, moving_average_decay=0.994,
                           teacher_temp=0.04).to(DEV)
    model.current_teacher_temp = 0.04
    g = torch.Generator().manual_seed(1)
    x = {"image": torch.rand(32, 3, 64, 64, generator=g).to(DEV), "tactile1": torch.rand(32, 3, 32, 32, generator=g).to(DEV),
         "tactile2": torch.rand(32, 3, 32, 32, generator=g).to(DEV)}
    out = model.training_step(x, 0)
    out["loss"].backward()
    torch.cuda.synchronize()
    grads = {n: p.grad.clone() for n, p in model.student_encoder.named_parameters() if p.grad is not None}
    model.on_train_batch_end(out, x, 0)
    return out["ssl_loss"], grads, model


@gpu
def test_full_size_reference_configuration_runs_and_repeats():
    """NOT a parity check: the reference configuration (K = 65536, B = 32, 2 + 8 views) goes through every kernel once in both compute
    types; loss and gradients are finite and two runs agree bit for bit.  The bf16 loss against the fp32 loss is printed, not asserted."""
    losses = {}
    for dt in ("fp32", "bf16"):
        loss_a, grads_a, model = _full_size_step(dt)
        assert np.isfinite(loss_a)
        assert len(grads_a) > 40
        for n, gr in grads_a.items():
            assert torch.isfinite(gr).all(), (dt, n)
        assert all(torch.isfinite(p).all() for p in model.teacher_encoder.parameters())
        del model
        loss_b, grads_b, model = _full_size_step(dt)
        del model
        assert loss_a == loss_b, (dt, loss_a, loss_b)
        for n in grads_a:
            assert torch.equal(grads_a[n], grads_b[n]), (dt, n)
        losses[dt] = loss_a
        del grads_a, grads_b
        torch.cuda.empty_cache()
    print(f"full size: loss fp32 {losses['fp32']:.6f}  bf16 {losses['bf16']:.6f}  rel difference {abs(losses['bf16'] - losses['fp32']) / abs(losses['fp32']):.3e}")
