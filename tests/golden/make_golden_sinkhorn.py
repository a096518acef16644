#!/usr/bin/env python3
"""Golden vectors of the Sinkhorn-Knopp teacher assignment (runs ONLY where the reference checkout is mounted; no test reads it).

Executes the REFERENCE's own `tactile_ssl/loss/dino_loss.py` DINOLoss.sinkhorn_knopp_teacher on the CPU, and its `models/vtdino.py`
step with the teacher-probability call routed to that method (what the `centering='sinkhorn_knopp'` branch of
`tactile_ssl/algorithm/dinov2.py` does: sinkhorn_knopp_teacher for the targets, no update_center), and writes data only:

  dino_sinkhorn.npz            per case `<name>/`: logits (Q, B, K) f32, teacher_temp, n_iterations, `ref32` the reference's output as it ran
                               (it casts to float32), `ref32_finite`, `f64` the same method run in float64, `ref32_err`, `log32_err`
  dino_sinkhorn_b35.npz        the (2, 35, 1000) case without its float64 result, dino_sinkhorn_b35_f64.npz that result (size limit of a
                               committed file; nothing recorded is left out)
  vtdino_sk_step.npz           two consecutive VTDINO steps on the STEP configuration of make_golden_vtdino.py (same seeds: the initial
                               parameters, inputs and masks are those of vtdino_step.npz and are not stored again): losses, bf16-operand
                               emulation errors
  vtdino_sk_step_s{1,2}.npz    per step: student and teacher logits, every student gradient

Logits.  Realistic cases are cosine logits normalize(x) @ (normalize(W) * g).T with g in [0.5, 1.5] (what DINOHead's weight-normalised last
layer produces), so |l| <= 1.5; D = 32.  The wide case is 2 * randn at teacher_temp 0.04: there exp(l / tt) overflows float32 and the
reference's own float32 run is not finite.

Errors.  float64: the reference's method with `Tensor.float()` returning float64 for the duration of the call (its only cast).
`ref32_err` = max |ref32 - f64| / f64.  `log32_err` = the same measure for a float32 torch run of the log-domain iteration
  z = L / tt, w = 0;  n times: u[k] = logsumexp_r(z[r,k] - w[r]), w[r] = logsumexp_k(z[r,k] - u[k]);  T = exp(z - u - w)
— the arithmetic the kernels restate.  For the wide case, whose probabilities reach 1e-40, both are measured as max |. - f64| / rowmax(f64)
instead (an elementwise relative error is ill-conditioned there); `<name>/err_measure` says which.

Usage:  python tests/golden/make_golden_sinkhorn.py
"""
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden_vtdino as MV  # noqa: E402

STEP = MV.STEP


class float_is_double:
    """Tensor.float() -> float64 while the reference's method runs: its arithmetic, in double."""

    def __enter__(self):
        self.real = torch.Tensor.float
        torch.Tensor.float = lambda t: t.double()

    def __exit__(self, *a):
        torch.Tensor.float = self.real


def sinkhorn_log_domain(logits, teacher_temp, n_iterations, dtype):
    z = logits.to(dtype) / teacher_temp
    w = torch.zeros(z.shape[0], dtype=dtype)
    u = None
    for _ in range(n_iterations):
        u = torch.logsumexp(z - w[:, None], dim=0)
        w = torch.logsumexp(z - u[None, :], dim=1)
    return torch.exp(z - u[None, :] - w[:, None])


def cosine_logits(g, rows, K, D=32):
    x = F.normalize(torch.randn(rows, D, generator=g), dim=-1)
    W = F.normalize(torch.randn(K, D, generator=g), dim=-1) * (0.5 + torch.rand(K, 1, generator=g))
    return x @ W.t()


def make_teacher_cases(DINOLoss):
    g = torch.Generator().manual_seed(23)
    small = cosine_logits(g, 6, 1000)
    big = cosine_logits(g, 70, 1000)
    wide = 2.0 * torch.randn(6, 1000, generator=g)
    cases = [("cos_b3_t04", small, (2, 3), 0.04, 3, "relative"), ("cos_b3_t07", small, (2, 3), 0.07, 3, "relative"),
             ("cos_b35_t07", big, (2, 35), 0.07, 3, "relative"), ("cos_b3_t04_it1", small, (2, 3), 0.04, 1, "relative"),
             ("wide_b3_t04", wide, (2, 3), 0.04, 3, "rowmax")]
    files = {"dino_sinkhorn.npz": {}, "dino_sinkhorn_b35.npz": {}, "dino_sinkhorn_b35_f64.npz": {}}
    names = []
    for name, logits, (Q, B), tt, n_it, measure in cases:
        K = logits.shape[1]
        assert float(logits.abs().max()) <= 1.5 or measure == "rowmax"
        loss = DINOLoss(out_dim=K)
        with np.errstate(all="ignore"):
            ref32 = loss.sinkhorn_knopp_teacher(logits.clone(), teacher_temp=tt, n_iterations=n_it).contiguous()
        assert ref32.dtype == torch.float32
        with float_is_double():
            f64 = loss.sinkhorn_knopp_teacher(logits.double(), teacher_temp=tt, n_iterations=n_it).contiguous()
        assert f64.dtype == torch.float64 and bool(torch.isfinite(f64).all())
        log64 = sinkhorn_log_domain(logits, tt, n_it, torch.float64)
        log32 = sinkhorn_log_domain(logits, tt, n_it, torch.float32)
        finite = bool(torch.isfinite(ref32).all())
        den = f64 if measure == "relative" else f64.amax(dim=1, keepdim=True)
        err = lambda t: float(((t.double() - f64).abs() / den).max())      # noqa: E731
        ref32_err = err(ref32) if finite else float("inf")
        log32_err = err(log32)
        restated = float(((log64 - f64).abs() / den).max())
        print(f"{name}: rows {Q * B} K {K} tt {tt} n {n_it}  ref32 finite {finite} err {ref32_err:.2e}  log32 err {log32_err:.2e}  "
              f"log-domain float64 vs reference float64 {restated:.2e}  smallest p {float(f64.min()):.2e}")
        main = files["dino_sinkhorn_b35.npz"] if name == "cos_b35_t07" else files["dino_sinkhorn.npz"]
        f64_file = files["dino_sinkhorn_b35_f64.npz"] if name == "cos_b35_t07" else main
        pre = name + "/"
        main[pre + "logits"] = logits.view(Q, B, K).numpy()
        main[pre + "teacher_temp"], main[pre + "n_iterations"] = np.float64(tt), np.int64(n_it)
        main[pre + "ref32"], main[pre + "ref32_finite"] = ref32.numpy(), np.bool_(finite)
        main[pre + "ref32_err"], main[pre + "log32_err"] = np.float64(ref32_err), np.float64(log32_err)
        main[pre + "err_measure"] = np.array(measure)
        f64_file[pre + "f64"] = f64.numpy()
        names.append(name)
    files["dino_sinkhorn.npz"]["cases"] = np.array(names)
    for f, d in files.items():
        np.savez_compressed(os.path.join(HERE, f), **d)


# ---- two steps with Sinkhorn-Knopp targets ----------------------------------------------------------------------------------------------
def route_to_sinkhorn(model, double):
    """softmax_center_teacher -> the reference's own sinkhorn_knopp_teacher on the ((q b), K) rows; update_center a no-op."""
    loss = model.dino_loss

    def teacher(t, teacher_temp):
        if double:
            with float_is_double():
                p = loss.sinkhorn_knopp_teacher(t.squeeze(1), teacher_temp=teacher_temp)
        else:
            p = loss.sinkhorn_knopp_teacher(t.squeeze(1), teacher_temp=teacher_temp)
        return p.contiguous().to(t.dtype).view(t.shape)
    loss.softmax_center_teacher = teacher
    loss.update_center = lambda t: None


def run_two_steps(model, x, dtype, emulate):
    model = model.to(dtype)
    route_to_sinkhorn(model, dtype == torch.float64)
    x = {k: v.to(dtype) for k, v in x.items()}
    cap = {}
    model.student_encoder["dino_head"].register_forward_hook(lambda m, i, o: cap.__setitem__("student", o.detach().clone()))
    model.teacher_encoder["dino_head"].register_forward_hook(lambda m, i, o: cap.__setitem__("teacher", o.detach().clone()))
    steps = []
    for s in range(2):
        for p in model.parameters():
            p.grad = None
        with MV.time_limit(60, f"step {s}"):
            if emulate:
                with MV.bf16_operands():
                    out = model.training_step(x, s)
                    out["loss"].backward()
            else:
                out = model.training_step(x, s)
                out["loss"].backward()
        rec = {"loss": float(out["loss"].detach())}
        st = cap["student"]
        rec["student_logits"] = st.permute(1, 0, 2).contiguous() if st.dim() == 3 else st
        rec["teacher_logits"] = cap["teacher"].reshape(STEP["n_global"], STEP["B"], -1)
        rec["grads"] = {n: p.grad.detach().clone() for n, p in model.student_encoder.named_parameters() if p.grad is not None}
        with torch.no_grad():
            for p in model.student_encoder.parameters():
                if p.grad is not None:
                    p.sub_(STEP["lr"] * p.grad)
        model.on_train_batch_end(out, x, s)
        assert float(model.dino_loss.center.abs().max()) == 0.0 and model.dino_loss.async_batch_center is None
        steps.append(rec)
    return steps


def make_step(vtt, vtd, DINOHead):
    f32 = lambda t: t.detach().to(torch.float32).numpy()   # noqa: E731
    model, x = MV.build_step_model(vtt, vtd, DINOHead)
    ref = run_two_steps(model, x, torch.float64, emulate=False)
    model2, x2 = MV.build_step_model(vtt, vtd, DINOHead)
    emu = run_two_steps(model2, x2, torch.float32, emulate=True)
    main = {}
    for s in range(2):
        r, e = ref[s], emu[s]
        main[f"step{s + 1}/loss"] = np.float64(r["loss"])
        np.savez_compressed(os.path.join(HERE, f"vtdino_sk_step_s{s + 1}.npz"), student_logits=f32(r["student_logits"]),
                            teacher_logits=f32(r["teacher_logits"]), **{"grad/" + n: f32(g) for n, g in r["grads"].items()})
        main[f"bf16emu/step{s + 1}/loss_rel"] = np.float64(abs(e["loss"] - r["loss"]) / abs(r["loss"]))
        names, emax, el2 = [], [], []
        for n, g in r["grads"].items():
            d = e["grads"][n].double() - g
            names.append(n)
            emax.append(float(d.abs().max() / g.abs().max().clamp_min(1e-30)))
            el2.append(float(d.norm() / g.norm().clamp_min(1e-30)))
        main[f"bf16emu/step{s + 1}/grad_names"] = np.array(names)
        main[f"bf16emu/step{s + 1}/grad_max_rel"] = np.array(emax)
        main[f"bf16emu/step{s + 1}/grad_rel_l2"] = np.array(el2)
        d = e["student_logits"].double() - r["student_logits"]
        main[f"bf16emu/step{s + 1}/student_logits_max_abs"] = np.float64(d.abs().max())
        d = e["teacher_logits"].double() - r["teacher_logits"]
        main[f"bf16emu/step{s + 1}/teacher_logits_max_abs"] = np.float64(d.abs().max())
        print(f"step {s + 1}: loss {r['loss']:.6f}  bf16-emulation loss rel {main[f'bf16emu/step{s + 1}/loss_rel']:.3e}  "
              f"grad max-rel worst {max(emax):.3e}  rel-L2 worst {max(el2):.3e}")
    np.savez_compressed(os.path.join(HERE, "vtdino_sk_step.npz"), **main)


if __name__ == "__main__":
    vtt, vtd, DINOHead, DINOLoss = MV.load_reference()
    make_teacher_cases(DINOLoss)
    make_step(vtt, vtd, DINOHead)
    for f in sorted(os.listdir(HERE)):
        if f.startswith(("dino_sinkhorn", "vtdino_sk")) and f.endswith(".npz"):
            print(f, os.path.getsize(os.path.join(HERE, f)))
