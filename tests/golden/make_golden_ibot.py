#!/usr/bin/env python3
"""Golden vectors of the iBOT patch loss (runs ONLY where the reference checkout is mounted; no test reads it).

Executes the REFERENCE's own `tactile_ssl/loss/ibot_patch_loss.py` iBOTPatchLoss on the CPU (`get_pylogger` stubbed, xformers absent, so its
`log_softmax` fallback), and its `models/vtdino.py` step with the patch term added exactly as `tactile_ssl/algorithm/dinov2.py` adds it (shared
head, scale 1 / num_global_masks, no KoLeo term), and writes data only:

  ibot_loss.npz, ibot_loss_<case>.npz   loss cases in float64, one file per case (size limit of a committed file).  The inputs are those of
                            tests/ibot_cases.py `inputs(Q, R, K)` and are pinned by their sha256 (`digest`), not stored: the float64 S, T, dS
                            and probabilities of one case are 4 to 80 MB.  Stored per case: the centre used, the loss, `pending` and the centre
                            after one update (the reference's (Q B, n, K) call, n = ibot_cases.SHAPES), and of dS, of the centred probabilities
                            and of the Sinkhorn-Knopp probabilities the rows ibot_cases.sample_rows names of every view in full plus, over ALL
                            rows, the column sums per view, the row 2-norms and the largest magnitude; the loss against the Sinkhorn-Knopp
                            targets.  On q3_r70_k1000 the Sinkhorn-Knopp call is recorded with n_masked_patches_tensor = 7 and = 1000: the
                            argument cancels (asserted here to 1e-15, pinned by test_ibot_cpu.py).
  vtdino_ibot_step.npz      two consecutive steps, centering="centering", on ISTEP (below): parameters, masks, total / DINO / patch losses, the
                            patch centre and its pending sums after each step, the bf16-operand emulation errors (make_golden_vtdino.py)
  vtdino_ibot_sk_step.npz   the same two steps with both terms' targets from sinkhorn_knopp_teacher (parameters, inputs and masks are the same
                            and not stored again)
  vtdino_ibot[_sk]_step_s{1,2}.npz     per step: register logits of student and teacher, every student gradient
  vtdino_ibot_step_inputs_<k>.npz      the three input tensors, one file each

Usage:  python tests/golden/make_golden_ibot.py
"""
import os
import sys

import einops
import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import ibot_cases as IC  # noqa: E402
import make_golden_sinkhorn as MS  # noqa: E402
import make_golden_vtdino as MV  # noqa: E402

ISTEP = dict(MV.STEP, size=64, B=8, n_global=2, global_scale=(0.5, 0.8), local_scale=(0.2, 0.35))
SK_TWICE = ((3, 70, 1000), (7, 1000))      # the case and the two values of n_masked_patches_tensor


def load_ibot():
    from tactile_ssl.loss.ibot_patch_loss import iBOTPatchLoss
    return iBOTPatchLoss


# ---- loss cases ----------------------------------------------------------------------------------------------------------------------------
def reference_case(iBOTPatchLoss, Q, R, K, n):
    S, T, c = IC.inputs(Q, R, K)
    B = R // n
    assert B * n == R
    mod = iBOTPatchLoss(patch_out_dim=K).double()
    mod.student_temp = IC.STUDENT_TEMP
    mod.center = c.double().view(1, 1, K).clone()
    S64 = S.double().requires_grad_(True)
    t_tokens = T.double().view(Q * B, n, K)                 # ((p b), k, c) as dinov2.py holds them
    probs = mod.softmax_center_teacher(t_tokens.unsqueeze(0), teacher_temp=IC.TEACHER_TEMP).squeeze(0)
    mod.update_center(t_tokens)
    probs = einops.rearrange(probs, "(p b) k c -> p b k c", p=Q, b=B)
    student = einops.rearrange(S64.view(Q * B, n, K), "(p b) k c -> p b k c", p=Q)
    loss = mod(list(student), list(probs))
    loss.backward()
    pending = mod.async_batch_center.reshape(K).clone()
    mod.apply_center_update()
    out = dict(loss=float(loss), dS=S64.grad.numpy(), probs=probs.reshape(Q, R, K).numpy(), pending=pending.numpy(),
               center_after=mod.center.reshape(K).numpy())
    # Sinkhorn-Knopp over all rows, as dinov2.py calls it: '(b k) c' rows, the scalar n
    sk = {}
    for n_masked in (SK_TWICE[1] if (Q, R, K) == SK_TWICE[0] else (n,)):
        with MS.float_is_double():
            p = mod.sinkhorn_knopp_teacher(T.double().view(Q * R, K), teacher_temp=IC.TEACHER_TEMP,
                                           n_masked_patches_tensor=torch.tensor(n_masked, dtype=int)).contiguous()
        assert p.dtype == torch.float64 and bool(torch.isfinite(p).all())
        sk[n_masked] = p.view(Q, R, K)
    first = next(iter(sk.values()))
    for p in sk.values():
        assert float((p - first).abs().max() / first.max()) <= 1e-15, "n_masked_patches_tensor changes the Sinkhorn-Knopp result"
    S2 = S.double().requires_grad_(True)
    loss_sk = mod(list(einops.rearrange(S2.view(Q * B, n, K), "(p b) k c -> p b k c", p=Q)),
                  list(einops.rearrange(first.reshape(Q * B, n, K), "(p b) k c -> p b k c", p=Q)))
    loss_sk.backward()
    out.update(sk={k: v.numpy() for k, v in sk.items()}, loss_sk=float(loss_sk), dS_sk=S2.grad.numpy())
    return (S, T, c), out


def make_cases(iBOTPatchLoss):
    index = {"cases": np.array([IC.case_name(*s) for s in IC.RECORDED]), "student_temp": np.float64(IC.STUDENT_TEMP),
             "teacher_temp": np.float64(IC.TEACHER_TEMP), "center_momentum": np.float64(IC.MOMENTUM)}
    for i, ((Q, R, K), n) in enumerate(IC.RECORDED.items()):
        (S, T, c), r = reference_case(iBOTPatchLoss, Q, R, K, n)
        rows = IC.sample_rows(R)
        name = IC.case_name(Q, R, K)
        d = {"dims": np.array([Q, R, K, n]), "digest": np.array(IC.digest(S, T, c)), "center_used": c.double().numpy(), "rows": np.array(rows),
             "loss": np.float64(r["loss"]), "loss_sk": np.float64(r["loss_sk"]), "pending": r["pending"], "center_after": r["center_after"]}
        sk_keys = list(r["sk"])
        d["sk_n_masked"] = np.array(sk_keys)
        for key, arr in (("dS", r["dS"]), ("probs", r["probs"]), ("sk", r["sk"][sk_keys[0]])):
            d[key + "/rows"] = arr[:, rows]
            d.update({f"{key}/{k}": v for k, v in IC.summaries(arr).items()})
        if len(sk_keys) > 1:
            d["sk_other/rows"] = r["sk"][sk_keys[1]][:, rows]
        d["dS_sk/rownorm"] = IC.summaries(r["dS_sk"])["rownorm"]
        mine = IC.ibot_f64(S, T, c, n)
        print(f"{name}: loss {r['loss']:.9f} (Sinkhorn-Knopp targets {r['loss_sk']:.9f})  restatement: loss rel {abs(mine['loss'] - r['loss']) / abs(r['loss']):.2e}  "
              f"dS {np.abs(mine['dS'] - r['dS']).max() / np.abs(r['dS']).max():.2e} of the largest entry  Sinkhorn-Knopp probabilities "
              f"{np.abs(IC.sinkhorn_f64(T)[0].reshape(Q, R, K) - next(iter(r['sk'].values()))).max() / next(iter(r['sk'].values())).max():.2e} of the largest")
        target = index if i == 0 else {}
        target.update({f"{name}/{k}": v for k, v in d.items()})
        if i:
            np.savez_compressed(os.path.join(HERE, f"ibot_loss_{name}.npz"), **target)
    np.savez_compressed(os.path.join(HERE, "ibot_loss.npz"), **index)


# ---- two steps with the patch term -----------------------------------------------------------------------------------------------------------
def build(vtt, vtd, DINOHead):
    step0 = MV.STEP
    MV.STEP = ISTEP
    try:
        model, x = MV.build_step_model(vtt, vtd, DINOHead)
    finally:
        MV.STEP = step0
    model.allow_mask_overlap = True     # as the reference's 2 + 8 view configuration: the global blocks keep all their patches (R = B x 3 x 36 or 49)
    return model, x


def _capture_first(backbone, cap, key):
    real = backbone.forward_features

    def forward_features(*a, **kw):
        out = real(*a, **kw)
        cap.setdefault(key, out)                            # the first call of a step: the global views
        return out
    backbone.forward_features = forward_features


def patch_term(model, ibot, cap, centering, double):
    """dinov2.py, forward: the lines that lead from the two global passes to `patch_loss`."""
    Q, tt = model.num_global_masks, model.current_teacher_temp
    s_tokens, t_tokens = cap["student"]["x_norm_patchtokens"], cap["teacher"]["x_norm_patchtokens"]
    B = s_tokens.shape[0] // Q
    student = model.student_encoder_dict["dino_head"](s_tokens)
    with torch.no_grad():
        teacher = model.teacher_encoder_dict["dino_head"](t_tokens)
        if centering == "centering":
            probs = ibot.softmax_center_teacher(teacher.unsqueeze(0), teacher_temp=tt).squeeze()
            ibot.update_center(teacher)
            probs = einops.rearrange(probs, "(p b) k c -> p b k c", p=Q, b=B)
        else:
            n_masked = teacher.shape[1]
            flat = einops.rearrange(teacher, "b k c -> (b k) c")
            kw = dict(teacher_temp=tt, n_masked_patches_tensor=torch.tensor(n_masked, dtype=int))
            if double:
                with MS.float_is_double():
                    probs = ibot.sinkhorn_knopp_teacher(flat, **kw)
            else:
                probs = ibot.sinkhorn_knopp_teacher(flat, **kw)
            probs = einops.rearrange(probs.contiguous().to(teacher.dtype).squeeze(), "(p b k) c -> p b k c", p=Q, b=B)
    student = einops.rearrange(student, "(p b) k c -> p b k c", p=Q)
    return (1.0 / Q) * ibot(list(student), list(probs)), s_tokens.shape[1]


def run_two_steps(model, x, dtype, emulate, iBOTPatchLoss, centering):
    model = model.to(dtype)
    if centering == "sinkhorn_knopp":
        MS.route_to_sinkhorn(model, dtype == torch.float64)
    ibot = iBOTPatchLoss(patch_out_dim=ISTEP["K"]).to(dtype)
    x = {k: v.to(dtype) for k, v in x.items()}
    cap, logits = {}, {}

    def keep_first(key):
        def hook(m, i, o):                                  # (a hook that returns a value would replace the head's output)
            if key not in logits:
                logits[key] = o.detach().clone()
        return hook
    model.student_encoder["dino_head"].register_forward_hook(keep_first("student"))
    model.teacher_encoder["dino_head"].register_forward_hook(keep_first("teacher"))
    _capture_first(model.student_encoder_dict["backbone"], cap, "student")
    _capture_first(model.teacher_encoder_dict["backbone"], cap, "teacher")
    steps = []
    for s in range(2):
        for p in model.parameters():
            p.grad = None
        cap.clear()
        logits.clear()

        def step():
            out = model.training_step(x, s)                 # the register logits are the heads' first calls of the step
            patch, n = patch_term(model, ibot, cap, centering, dtype == torch.float64)
            total = out["loss"] + patch
            total.backward()
            return out, float(out["loss"].detach()), float(patch.detach()), float(total.detach()), n
        with MV.time_limit(300, f"step {s}"):
            if emulate:
                with MV.bf16_operands():
                    out, dino, patch, total, n = step()
            else:
                out, dino, patch, total, n = step()
        rec = {"loss": total, "dino": dino, "ibot": patch, "n": n}
        st = logits["student"]
        rec["student_logits"] = st.permute(1, 0, 2).contiguous() if st.dim() == 3 else st
        rec["teacher_logits"] = logits["teacher"].reshape(ISTEP["n_global"], ISTEP["B"], -1)
        rec["grads"] = {k: p.grad.detach().clone() for k, p in model.student_encoder.named_parameters() if p.grad is not None}
        rec["unused"] = [k for k, p in model.student_encoder.named_parameters() if p.grad is None]
        assert all(p.grad is None for p in model.teacher_encoder.parameters())
        with torch.no_grad():
            for p in model.student_encoder.parameters():
                if p.grad is not None:
                    p.sub_(ISTEP["lr"] * p.grad)
        model.on_train_batch_end(out, x, s)
        if centering == "centering":
            rec["pending"] = ibot.async_batch_center.detach().reshape(-1).clone()
            rec["center_before"] = ibot.center.detach().reshape(-1).clone()     # the centre this step's targets used
        else:
            assert float(ibot.center.abs().max()) == 0.0 and ibot.async_batch_center is None
        steps.append(rec)
    return steps


def make_step(vtt, vtd, DINOHead, iBOTPatchLoss, centering, stem, with_inputs):
    f32 = lambda t: t.detach().to(torch.float32).numpy()   # noqa: E731
    model, x = build(vtt, vtd, DINOHead)
    main = {"meta/" + k: np.asarray(v) for k, v in ISTEP.items()}
    main["meta/centering"], main["meta/allow_mask_overlap"] = np.array(centering), np.bool_(True)
    if with_inputs:
        sd = model.state_dict()
        main["keys"] = np.array(list(sd.keys()))
        for k, v in sd.items():
            if k.startswith("student_encoder.") or k.startswith("teacher_encoder.dino_head.") or k.startswith("dino_loss."):
                main["param/" + k] = f32(v)
        for k, v in x.items():
            np.savez_compressed(os.path.join(HERE, f"{stem}_inputs_{k}.npz"), **{"input/" + k: f32(v)})
        for s in range(2):
            model.generator.manual_seed(s)
            gm, lm = model.sample_masks(x["image"])
            for i, m in enumerate(gm):
                main[f"mask/{s}/global/{i}"] = m.numpy()
            for i, m in enumerate(lm):
                main[f"mask/{s}/local/{i}"] = m.numpy()
    ref = run_two_steps(model, x, torch.float64, False, iBOTPatchLoss, centering)
    model2, x2 = build(vtt, vtd, DINOHead)
    emu = run_two_steps(model2, x2, torch.float32, True, iBOTPatchLoss, centering)
    for s in range(2):
        r, e = ref[s], emu[s]
        pre = f"step{s + 1}/"
        main[pre + "loss"], main[pre + "dino_loss"], main[pre + "ibot_loss"] = np.float64(r["loss"]), np.float64(r["dino"]), np.float64(r["ibot"])
        main[pre + "patches_per_view_row"] = np.int64(r["n"])
        main[pre + "unused_params"] = np.array(r["unused"])
        if centering == "centering":
            main[pre + "ibot_pending"], main[pre + "ibot_center_used"] = f32(r["pending"]), f32(r["center_before"])
        np.savez_compressed(os.path.join(HERE, f"{stem}_s{s + 1}.npz"), student_logits=f32(r["student_logits"]),
                            teacher_logits=f32(r["teacher_logits"]), **{"grad/" + k: f32(g) for k, g in r["grads"].items()})
        main[f"bf16emu/{pre}loss_rel"] = np.float64(abs(e["loss"] - r["loss"]) / abs(r["loss"]))
        main[f"bf16emu/{pre}ibot_rel"] = np.float64(abs(e["ibot"] - r["ibot"]) / abs(r["ibot"]))
        names, emax, el2 = [], [], []
        for k, g in r["grads"].items():
            d = e["grads"][k].double() - g
            names.append(k)
            emax.append(float(d.abs().max() / g.abs().max().clamp_min(1e-30)))
            el2.append(float(d.norm() / g.norm().clamp_min(1e-30)))
        main[f"bf16emu/{pre}grad_names"] = np.array(names)
        main[f"bf16emu/{pre}grad_max_rel"] = np.array(emax)
        main[f"bf16emu/{pre}grad_rel_l2"] = np.array(el2)
        main[f"bf16emu/{pre}student_logits_max_abs"] = np.float64((e["student_logits"].double() - r["student_logits"]).abs().max())
        main[f"bf16emu/{pre}teacher_logits_max_abs"] = np.float64((e["teacher_logits"].double() - r["teacher_logits"]).abs().max())
        print(f"[{centering}] step {s + 1}: loss {r['loss']:.6f} = dino {r['dino']:.6f} + ibot {r['ibot']:.6f}  R = {ISTEP['B']} x {r['n']}  bf16-emulation "
              f"loss rel {main[f'bf16emu/{pre}loss_rel']:.3e}  grad max-rel worst {max(emax):.3e}  rel-L2 worst {max(el2):.3e}")
    np.savez_compressed(os.path.join(HERE, stem + ".npz"), **main)


if __name__ == "__main__":
    vtt, vtd, DINOHead, _ = MV.load_reference()
    iBOTPatchLoss = load_ibot()
    make_cases(iBOTPatchLoss)
    make_step(vtt, vtd, DINOHead, iBOTPatchLoss, "centering", "vtdino_ibot_step", True)
    make_step(vtt, vtd, DINOHead, iBOTPatchLoss, "sinkhorn_knopp", "vtdino_ibot_sk_step", False)
    for f in sorted(os.listdir(HERE)):
        if f.startswith(("ibot_loss", "vtdino_ibot")) and f.endswith(".npz"):
            print(f, os.path.getsize(os.path.join(HERE, f)))
