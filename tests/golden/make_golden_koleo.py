#!/usr/bin/env python3
"""Golden vectors of the KoLeo regulariser (runs ONLY where the reference checkout is mounted; no test reads it).

Executes the REFERENCE's own `tactile_ssl/loss/koleo_loss.py` KoLeoLoss on the CPU (the class imports only torch), and its `models/vtdino.py`
step with `koleo_weight * sum over global views of KoLeoLoss(student register rows of the view)` added to the loss (what
`tactile_ssl/algorithm/dinov2.py` adds: KoLeo on each chunk of the student's global class tokens), and writes data only:

  dino_koleo.npz            per case `<name>/`: x (n, D) f32; `loss64`, `grad64`, `indices` the class run in float64; `loss32`, `grad32` the
                            class as it runs (float32); `loss32_err` = |loss32 - loss64| / max(1, |loss64|), `grad32_err` = max |grad32 - grad64| /
                            max |grad64|; `gap` the smallest float64 margin between a row's best product and the next one that is not exactly equal
  vtdino_koleo_step.npz     two consecutive VTDINO steps in float64 on KSTEP (below) with its own parameters, inputs and masks: total, DINO and
                            weighted KoLeo losses, the per-view neighbours, the margin records, and the bf16-operand emulation errors
  vtdino_koleo_step_s{1,2}.npz   per step: student and teacher logits, every student gradient
  vtdino_koleo_step_inputs.npz   the three input tensors (a file of their own: the size limit of a committed file; nothing recorded is left out)

Cases.  (1, 192) and (2, 192); (6, 192) with rows 0, 1 and 4 identical (exact ties: the lowest index wins, and d = sqrt(D) 1e-8 there);
(5, 64) with row 2 zero (clamped norm, every product 0); torch.randn from seed 0 at (35, 256), (64, 192), (67, 100), (33, 50); the planted
construction of tests/koleo_cases.py at (130, 256).  Every input satisfies koleo_cases.neighbour_gap (asserted here), and the reference's float32
run picks the float64 neighbours in every case (asserted here).

Step.  The register rows of the student's global views are captured from the student backbone's first forward_features call of each step
(the reference runs the global views first).  They are nearly collinear, so a neighbour is decided by products that differ in the fourth
digit, and the bf16 mode perturbs them in the fifth: the input seed is the first of 101, 102, ... (at most 32) for which, at both steps and in
both views, the float64 margin is at least 10 times the largest difference between the products of the bf16-emulated run and of the
float64 run, and the emulated run picks the float64 neighbours.  `margin/...` records the figures of the chosen seed.

Usage:  python tests/golden/make_golden_koleo.py
"""
import importlib.util
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import koleo_cases as KC  # noqa: E402
import make_golden_vtdino as MV  # noqa: E402

KSTEP = dict(MV.STEP, size=64, B=6, n_global=2, global_scale=(0.5, 0.8), local_scale=(0.2, 0.35), koleo_weight=0.1)
MARGIN = 10.0
SEEDS = range(101, 133)


def load_koleo():
    spec = importlib.util.spec_from_file_location("ref_koleo_loss", os.path.join(MV.REF, "tactile_ssl", "loss", "koleo_loss.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m.KoLeoLoss


def loss_cases():
    g = torch.Generator().manual_seed(5)
    tie = torch.randn(6, 192, generator=g)
    tie[1] = tie[0]
    tie[4] = tie[0]
    zero = torch.randn(5, 64, generator=g)
    zero[2] = 0
    cases = [("single_1x192", torch.randn(1, 192, generator=g)), ("pair_2x192", torch.randn(2, 192, generator=g)), ("tie_6x192", tie),
             ("zero_5x64", zero)]
    cases += [(f"randn_{n}x{D}", KC.random_rows(n, D, 0)) for n, D in KC.RANDOM_SHAPES]
    cases.append(("planted_130x256", KC.planted_rows(130, 256, 0)[0]))
    return cases


def run_class(KoLeoLoss, x):
    x = x.clone().requires_grad_(True)
    mod = KoLeoLoss()
    loss = mod(x)
    loss.backward()
    with torch.no_grad():
        idx = mod.pairwise_NNs_inner(torch.nn.functional.normalize(x, eps=1e-8, p=2, dim=-1))
    return loss.detach(), x.grad, idx


def make_cases(KoLeoLoss):
    out, names = {}, []
    for name, x in loss_cases():
        gap = KC.neighbour_gap(x.numpy())
        l64, g64, i64 = run_class(KoLeoLoss, x.double())
        l32, g32, i32 = run_class(KoLeoLoss, x)
        assert l64.dtype == torch.float64 and l32.dtype == torch.float32
        assert torch.equal(i64, i32), f"{name}: the reference's float32 run picks other neighbours than its float64 run"
        r = KC.koleo_f64(x.numpy())
        assert np.array_equal(r["indices"], i64.numpy()), name
        l_err = abs(float(l32) - float(l64)) / max(1.0, abs(float(l64)))
        g_err = float((g32.double() - g64).abs().max() / g64.abs().max().clamp_min(1e-300))
        pre = name + "/"
        out[pre + "x"] = x.numpy()
        out[pre + "loss64"], out[pre + "grad64"], out[pre + "indices"] = np.float64(l64), g64.numpy(), i64.numpy()
        out[pre + "loss32"], out[pre + "grad32"] = np.float32(l32), g32.numpy()
        out[pre + "loss32_err"], out[pre + "grad32_err"], out[pre + "gap"] = np.float64(l_err), np.float64(g_err), np.float64(gap)
        names.append(name)
        print(f"{name}: loss {float(l64):.6f}  f32 loss err {l_err:.2e} grad err {g_err:.2e}  gap {gap:.2e}  max in-degree {KC.in_degree(i64.numpy()).max()}  "
              f"largest |grad| {float(g64.abs().max()):.3e}")
    out["cases"] = np.array(names)
    np.savez_compressed(os.path.join(HERE, "dino_koleo.npz"), **out)


# ---- two steps with the KoLeo term ---------------------------------------------------------------------------------------------------------
def build(vtt, vtd, DINOHead, input_seed):
    MV.STEP = KSTEP
    try:
        model, x = MV.build_step_model(vtt, vtd, DINOHead)
    finally:
        MV.STEP = STEP0
    g = torch.Generator().manual_seed(input_seed)
    B = KSTEP["B"]
    x = {k: v * (0.25 + 1.5 * torch.rand(B, 1, 1, 1, generator=g)) + 0.3 * torch.randn(B, 3, 1, 1, generator=g) for k, v in x.items()}
    return model, x


STEP0 = MV.STEP


def run_two_steps(model, x, dtype, emulate, KoLeoLoss):
    model = model.to(dtype)
    x = {k: v.to(dtype) for k, v in x.items()}
    Q, B, w = KSTEP["n_global"], KSTEP["B"], KSTEP["koleo_weight"]
    cap = {}
    model.student_encoder["dino_head"].register_forward_hook(lambda m, i, o: cap.__setitem__("student", o.detach().clone()))
    model.teacher_encoder["dino_head"].register_forward_hook(lambda m, i, o: cap.__setitem__("teacher", o.detach().clone()))
    backbone = model.student_encoder_dict["backbone"]
    real_ff = backbone.forward_features

    def forward_features(*a, **kw):
        out = real_ff(*a, **kw)
        cap.setdefault("rows", out["x_norm_regtokens"])            # the first call of a step: the global views, ((p b), 1, c)
        return out
    backbone.forward_features = forward_features
    koleo = KoLeoLoss()
    steps = []
    for s in range(2):
        for p in model.parameters():
            p.grad = None
        cap.pop("rows", None)

        def step():
            out = model.training_step(x, s)
            rows = cap["rows"][:, 0]
            assert rows.shape[0] == Q * B and rows.requires_grad
            kl = sum(koleo(rows[v * B:(v + 1) * B]) for v in range(Q))
            total = out["loss"] + w * kl
            total.backward()
            return out, rows.detach().clone(), float(out["loss"].detach()), float(w * kl.detach()), float(total.detach())
        with MV.time_limit(120, f"step {s}"):
            if emulate:
                with MV.bf16_operands():
                    out, rows, dino, kl, total = step()
            else:
                out, rows, dino, kl, total = step()
        rec = {"loss": total, "dino": dino, "koleo": kl, "rows": rows.view(Q, B, -1)}
        st = cap["student"]
        rec["student_logits"] = st.permute(1, 0, 2).contiguous() if st.dim() == 3 else st
        rec["teacher_logits"] = cap["teacher"].reshape(Q, B, -1)
        rec["grads"] = {n: p.grad.detach().clone() for n, p in model.student_encoder.named_parameters() if p.grad is not None}
        rec["unused"] = [n for n, p in model.student_encoder.named_parameters() if p.grad is None]
        with torch.no_grad():
            for p in model.student_encoder.parameters():
                if p.grad is not None:
                    p.sub_(KSTEP["lr"] * p.grad)
        model.on_train_batch_end(out, x, s)
        steps.append(rec)
    backbone.forward_features = real_ff
    return steps


def margins(ref, emu):
    """Per step and view: (float64 margin, largest |emulated product - float64 product|, neighbours of both runs)."""
    out = []
    for r, e in zip(ref, emu):
        for v in range(KSTEP["n_global"]):
            x64, xe = r["rows"][v].double().numpy(), e["rows"][v].double().numpy()
            gap = _raw_gap(x64)
            y64, ye = KC._normalized(x64, 1e-8)[0], KC._normalized(xe, 1e-8)[0]
            diff = float(np.abs(ye @ ye.T - y64 @ y64.T).max())
            out.append((gap, diff, KC.koleo_f64(x64)["indices"], KC.koleo_f64(xe)["indices"]))
    return out


def _raw_gap(x):
    dots = KC._products(KC._normalized(x, 1e-8)[0])
    top = np.sort(dots, axis=1)[:, -2:]
    return float((top[:, 1] - top[:, 0]).min())


def make_step(vtt, vtd, DINOHead, KoLeoLoss):
    f32 = lambda t: t.detach().to(torch.float32).numpy()   # noqa: E731
    chosen, both_steps = None, True
    first_step_only = None
    for seed in SEEDS:
        model, x = build(vtt, vtd, DINOHead, seed)
        ref = run_two_steps(model, x, torch.float64, False, KoLeoLoss)
        model2, x2 = build(vtt, vtd, DINOHead, seed)
        emu = run_two_steps(model2, x2, torch.float32, True, KoLeoLoss)
        mg = margins(ref, emu)
        ok = [gap >= KC.GAP and gap >= MARGIN * diff and np.array_equal(i64, ie) for gap, diff, i64, ie in mg]
        print(f"input seed {seed}: " + "  ".join(f"gap {gap:.2e} / product diff {diff:.2e} = {gap / diff:.1f}x {'ok' if o else 'NO'}"
                                                for (gap, diff, _, _), o in zip(mg, ok)))
        if all(ok):
            chosen = (seed, ref, emu, mg)
            break
        if first_step_only is None and all(ok[:KSTEP["n_global"]]):
            first_step_only = (seed, ref, emu, mg)
    if chosen is None:
        assert first_step_only is not None, "no input seed passes even the first step"
        chosen, both_steps = first_step_only, False
    seed, ref, emu, mg = chosen
    n_steps = 2 if both_steps else 1
    model, x = build(vtt, vtd, DINOHead, seed)
    main = {"meta/" + k: np.asarray(v) for k, v in KSTEP.items()}
    main["meta/input_seed"], main["meta/steps"] = np.int64(seed), np.int64(n_steps)
    sd = model.state_dict()
    main["keys"] = np.array(list(sd.keys()))
    for k, v in sd.items():
        if k.startswith("student_encoder.") or k.startswith("teacher_encoder.dino_head.") or k.startswith("dino_loss."):
            main["param/" + k] = f32(v)
    np.savez_compressed(os.path.join(HERE, "vtdino_koleo_step_inputs.npz"), **{"input/" + k: f32(v) for k, v in x.items()})
    for s in range(n_steps):
        model.generator.manual_seed(s)
        gm, lm = model.sample_masks(x["image"])
        assert not torch.equal(gm[0], gm[1]), "the two global masks are the same"
        for i, m in enumerate(gm):
            main[f"mask/{s}/global/{i}"] = m.numpy()
        for i, m in enumerate(lm):
            main[f"mask/{s}/local/{i}"] = m.numpy()
    Q = KSTEP["n_global"]
    for s in range(n_steps):
        r, e = ref[s], emu[s]
        main[f"step{s + 1}/loss"], main[f"step{s + 1}/dino_loss"] = np.float64(r["loss"]), np.float64(r["dino"])
        main[f"step{s + 1}/koleo_loss"] = np.float64(r["koleo"])
        main[f"step{s + 1}/koleo_indices"] = np.stack([mg[s * Q + v][2] for v in range(Q)])
        main[f"step{s + 1}/unused_params"] = np.array(r["unused"])
        main[f"margin/step{s + 1}/gap"] = np.array([mg[s * Q + v][0] for v in range(Q)])
        main[f"margin/step{s + 1}/bf16_product_diff"] = np.array([mg[s * Q + v][1] for v in range(Q)])
        np.savez_compressed(os.path.join(HERE, f"vtdino_koleo_step_s{s + 1}.npz"), student_logits=f32(r["student_logits"]),
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
        main[f"bf16emu/step{s + 1}/student_logits_max_abs"] = np.float64((e["student_logits"].double() - r["student_logits"]).abs().max())
        main[f"bf16emu/step{s + 1}/teacher_logits_max_abs"] = np.float64((e["teacher_logits"].double() - r["teacher_logits"]).abs().max())
        print(f"step {s + 1}: loss {r['loss']:.6f} = dino {r['dino']:.6f} + koleo {r['koleo']:.6f}  bf16-emulation loss rel "
              f"{main[f'bf16emu/step{s + 1}/loss_rel']:.3e}  grad max-rel worst {max(emax):.3e}  rel-L2 worst {max(el2):.3e}")
    np.savez_compressed(os.path.join(HERE, "vtdino_koleo_step.npz"), **main)


if __name__ == "__main__":
    KoLeoLoss = load_koleo()
    make_cases(KoLeoLoss)
    vtt, vtd, DINOHead, _ = MV.load_reference()
    make_step(vtt, vtd, DINOHead, KoLeoLoss)
    for f in sorted(os.listdir(HERE)):
        if f.startswith(("dino_koleo", "vtdino_koleo")) and f.endswith(".npz"):
            print(f, os.path.getsize(os.path.join(HERE, f)))
