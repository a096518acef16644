#!/usr/bin/env python3
"""Golden vectors of the DINO self-distillation step (runs ONLY where the reference checkout is mounted; no test reads it).

Executes the REFERENCE's own classes on the CPU — `models/vtdino.py` (VTDINO), `models/VTT.py` (the DINO-style encoder),
`tactile_ssl/model/layers/dino_head.py` (DINOHead), `tactile_ssl/loss/dino_loss.py` (DINOLoss), `tactile_ssl/utils/ema.py` — imported
from where they lie with the stubs of make_golden.py plus two more (an `omegaconf` exposing ListConfig, a `tactile_ssl.algorithm`
exposing an empty Module), and writes data only:

  vtdino_step.npz            initial parameters of both networks (the teacher backbone starts as a copy of the student's, so only the
                             teacher's head is stored), inputs, sampled masks, the losses, the centre and its pending sums after each of two
                             consecutive steps, the recorded schedules, and the errors of the bf16-operand emulation (below)
  vtdino_step_s{1,2}.npz     per step: student and teacher logits, every student gradient
  vtdino_teacher_s{1,2}.npz  per step: every teacher parameter after on_train_batch_end
  vtdino_masks.npz           sample_masks output for several step seeds on the 8x8 and the 4x4 grid
  dino_head_init.npz         seeded initial state dicts of small heads, forward / backward on a fixed input
  dino_loss_f64.npz          DINOLoss in float64, two consecutive calls, non-zero centre

The step runs in float64 (the model's seeded float32 initial values, `.double()`), stored rounded to float32 once: one yardstick for
the fp32 and the bf16 mode.  Between the steps the student takes a plain SGD update.  (One file would pass the size limit of a committed
file, hence the split; nothing recorded is left out.)

bf16 emulation: the same two steps once more in float32 with every matrix product's operands rounded to bfloat16 where the kernels
round them — both operands of every nn.Linear (the weight-normalised prototype layer included) and of the two attention products,
forwards, and the incoming gradient and the saved operands of each, backwards.  Its error against the float64 run is recorded per
parameter (`bf16emu/...`); the GPU test takes twice the largest recorded value of a step as that step's bound.

Usage:  python tests/golden/make_golden_vtdino.py
"""
import importlib.util
import os
import signal
import sys
import types
from functools import partial

import numpy as np
import torch
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as MG  # noqa: E402

REF = MG.REF          # where the reference checkout is mounted (make_golden.py)


def load_reference():
    MG._install_stubs()
    sys.path.insert(0, REF)

    class ListConfig(list):
        pass
    sys.modules["omegaconf"].ListConfig = ListConfig
    import tactile_ssl  # noqa: F401
    pkg = types.ModuleType("tactile_ssl.model")
    pkg.__path__ = [os.path.join(REF, "tactile_ssl", "model")]
    sys.modules["tactile_ssl.model"] = pkg
    alg = types.ModuleType("tactile_ssl.algorithm")
    alg.Module = type("Module", (), {})
    sys.modules["tactile_ssl.algorithm"] = alg

    def load(name, rel):
        spec = importlib.util.spec_from_file_location(name, os.path.join(REF, rel))
        m = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(m)
        return m
    vtt = load("ref_VTT", "models/VTT.py")
    vtd = load("ref_vtdino", "models/vtdino.py")
    from tactile_ssl.loss.dino_loss import DINOLoss
    from tactile_ssl.model.layers.dino_head import DINOHead
    return vtt, vtd, DINOHead, DINOLoss


class time_limit:
    def __init__(self, seconds, what):
        self.seconds, self.what = seconds, what

    def __enter__(self):
        def handler(signum, frame):
            raise RuntimeError(f"{self.what}: the reference did not return within {self.seconds} s")
        signal.signal(signal.SIGALRM, handler)
        signal.alarm(self.seconds)

    def __exit__(self, *a):
        signal.alarm(0)


# ---- bf16-operand emulation ----------------------------------------------------------------------------------------------------------
def _r(x):
    return x.to(torch.bfloat16).to(x.dtype)


_real_linear, _real_matmul = F.linear, torch.matmul


class _LinearBf16(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, w, b):
        xr, wr = _r(x), _r(w)
        ctx.save_for_backward(xr, wr)
        ctx.has_b = b is not None
        return _real_linear(xr, wr, b)

    @staticmethod
    def backward(ctx, dy):
        xr, wr = ctx.saved_tensors
        d = _r(dy)
        d2, x2 = d.reshape(-1, d.shape[-1]), xr.reshape(-1, xr.shape[-1])
        return _real_matmul(d, wr), _real_matmul(d2.t(), x2), d2.sum(0) if ctx.has_b else None


class _MatmulBf16(torch.autograd.Function):
    @staticmethod
    def forward(ctx, a, b):
        ar, br = _r(a), _r(b)
        ctx.save_for_backward(ar, br)
        return _real_matmul(ar, br)

    @staticmethod
    def backward(ctx, dy):
        ar, br = ctx.saved_tensors
        d = _r(dy)
        return _real_matmul(d, br.transpose(-1, -2)), _real_matmul(ar.transpose(-1, -2), d)


class bf16_operands:
    def __enter__(self):
        F.linear = lambda x, w, b=None: _LinearBf16.apply(x, w, b)
        torch.matmul = lambda a, b: _MatmulBf16.apply(a, b)

    def __exit__(self, *a):
        F.linear, torch.matmul = _real_linear, _real_matmul


# ---- fixture 1: two steps ------------------------------------------------------------------------------------------------------------
STEP = dict(dim=64, depth=1, heads=1, mlp=128, size=32, patch=8, hidden=64, bottleneck=32, K=1024, B=4, n_global=1, n_local=4,
            local_scale=(0.45, 0.6), global_scale=(0.7, 1.0), min_keep=4, teacher_temp=0.05, decay=0.9, lr=0.05, seed=31)


def build_step_model(vtt, vtd, DINOHead):
    c = STEP
    torch.manual_seed(c["seed"])
    enc = vtt.VTT(image_size=c["size"], tactile_size=c["size"], image_patch_size=c["patch"], tactile_patch_size=c["patch"], dim=c["dim"],
                  depth=c["depth"], heads=c["heads"], mlp_dim=c["mlp"], num_tactiles=2, num_register_tokens=1)
    g = torch.Generator().manual_seed(c["seed"] + 1)
    with torch.no_grad():                       # make LayerNorm affine terms, biases and the register token matter
        for _, p in enc.named_parameters():
            if p.dim() == 1:
                p.add_(0.1 * torch.randn(p.shape, generator=g))
        enc.register_tokens.add_(0.5 * torch.randn(enc.register_tokens.shape, generator=g))
    model = vtd.VTDINO(encoder=enc, dino_head=partial(DINOHead, out_dim=c["K"], hidden_dim=c["hidden"], bottleneck_dim=c["bottleneck"]),
                       optim_cfg=None, lr_scheduler_cfg=None, wd_scheduler_cfg=None, local_mask_scale=c["local_scale"],
                       global_mask_scale=c["global_scale"], num_global_masks=c["n_global"], num_local_masks=c["n_local"],
                       min_keep_num_sensors=c["min_keep"], allow_mask_overlap=False, moving_average_decay=c["decay"],
                       teacher_temp=c["teacher_temp"])
    with torch.no_grad():
        for net in (model.student_encoder, model.teacher_encoder):
            head = net["dino_head"]
            head.last_layer.weight_g.add_(0.2 * torch.randn(head.last_layer.weight_g.shape, generator=g))
            for n_, p in head.named_parameters():
                if n_.endswith("bias"):
                    p.add_(0.05 * torch.randn(p.shape, generator=g))
    model.current_teacher_temp = c["teacher_temp"]
    x = {k: torch.rand(c["B"], 3, c["size"], c["size"], generator=g) for k in ("image", "tactile1", "tactile2")}
    return model, x


def run_two_steps(model, x, dtype, emulate):
    model = model.to(dtype)
    x = {k: v.to(dtype) for k, v in x.items()}
    cap = {}
    model.student_encoder["dino_head"].register_forward_hook(lambda m, i, o: cap.__setitem__("student", o.detach().clone()))
    model.teacher_encoder["dino_head"].register_forward_hook(lambda m, i, o: cap.__setitem__("teacher", o.detach().clone()))
    steps = []
    for s in range(2):
        for p in model.parameters():
            p.grad = None
        with time_limit(60, f"step {s}"):
            if emulate:
                with bf16_operands():
                    out = model.training_step(x, s)
                    out["loss"].backward()
            else:
                out = model.training_step(x, s)
                out["loss"].backward()
        rec = {"loss": float(out["loss"].detach())}
        # (p b) rows of the student as (P, B, K): the reference feeds the head (b, p, c)
        st = cap["student"]
        rec["student_logits"] = st.permute(1, 0, 2).contiguous() if st.dim() == 3 else st
        rec["teacher_logits"] = cap["teacher"].reshape(STEP["n_global"], STEP["B"], -1)
        rec["grads"] = {n: p.grad.detach().clone() for n, p in model.student_encoder.named_parameters() if p.grad is not None}
        rec["unused"] = [n for n, p in model.student_encoder.named_parameters() if p.grad is None]
        assert all(p.grad is None for p in model.teacher_encoder.parameters())
        with torch.no_grad():
            for p in model.student_encoder.parameters():
                if p.grad is not None:
                    p.sub_(STEP["lr"] * p.grad)
        model.on_train_batch_end(out, x, s)
        rec["center"] = model.dino_loss.center.detach().clone()
        rec["pending"] = model.dino_loss.async_batch_center.detach().clone()
        rec["teacher"] = {n: p.detach().clone() for n, p in model.teacher_encoder.named_parameters()}
        steps.append(rec)
    return steps


def make_step(vtt, vtd, DINOHead):
    f32 = lambda t: t.detach().to(torch.float32).numpy()   # noqa: E731
    model, x = build_step_model(vtt, vtd, DINOHead)
    main = {"meta/" + k: np.asarray(v) for k, v in STEP.items()}
    sd = model.state_dict()
    main["keys"] = np.array(list(sd.keys()))
    main["shapes"] = np.array([",".join(str(d) for d in v.shape) for v in sd.values()])
    for k, v in sd.items():
        if k.startswith("student_encoder.") or k.startswith("teacher_encoder.dino_head.") or k.startswith("dino_loss."):
            main["param/" + k] = f32(v)
    for k, v in x.items():
        main["input/" + k] = f32(v)
    # masks of the two steps (training_step seeds the generator with the step counter 0, 1)
    for s in range(2):
        model.generator.manual_seed(s)
        gm, lm = model.sample_masks(x["image"])
        for i, m in enumerate(gm):
            main[f"mask/{s}/global/{i}"] = m.numpy()
        for i, m in enumerate(lm):
            main[f"mask/{s}/local/{i}"] = m.numpy()
    ref = run_two_steps(model, x, torch.float64, emulate=False)
    model2, x2 = build_step_model(vtt, vtd, DINOHead)
    emu = run_two_steps(model2, x2, torch.float32, emulate=True)
    for s in range(2):
        r, e = ref[s], emu[s]
        main[f"step{s + 1}/loss"] = np.float64(r["loss"])
        main[f"step{s + 1}/center"] = f32(r["center"])
        main[f"step{s + 1}/pending"] = f32(r["pending"])
        main[f"step{s + 1}/unused_params"] = np.array(r["unused"])
        np.savez_compressed(os.path.join(HERE, f"vtdino_step_s{s + 1}.npz"), student_logits=f32(r["student_logits"]),
                            teacher_logits=f32(r["teacher_logits"]), **{"grad/" + n: f32(g) for n, g in r["grads"].items()})
        np.savez_compressed(os.path.join(HERE, f"vtdino_teacher_s{s + 1}.npz"), **{"teacher/" + n: f32(p) for n, p in r["teacher"].items()})
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
    # schedules of the reference's generators
    sched = vtd.VTDINO(encoder=model.student_encoder["backbone"], dino_head=partial(DINOHead, out_dim=64, hidden_dim=32, bottleneck_dim=16),
                       optim_cfg=lambda groups: torch.optim.SGD(groups, lr=0.1), lr_scheduler_cfg=lambda **kw: None, wd_scheduler_cfg=None,
                       moving_average_decay=[0.99, 1.0], teacher_temp=[0.04, 0.07], teacher_warmup_epochs=1)
    opt, _, _ = sched.configure_optimizers(5, 3)
    main["sched/args"] = np.array([5, 3, 1])
    main["sched/teacher_temp"] = np.array(list(sched.teacher_temp_scheduler), dtype=np.float64)
    main["sched/momentum"] = np.array(list(sched.momentum_scheduler), dtype=np.float64)
    main["sched/group_sizes"] = np.array([len(g["params"]) for g in opt.param_groups])
    np.savez_compressed(os.path.join(HERE, "vtdino_step.npz"), **main)


# ---- fixture 2: masks ----------------------------------------------------------------------------------------------------------------
def make_masks(vtt, vtd, DINOHead):
    out = {}
    cases = {"grid8": dict(size=64, patch=8, B=8, seeds=list(range(8)), n_global=2, n_local=8, global_scale=(0.48, 1.0),
                           local_scale=(0.2, 0.48), overlap=True, min_keep=4),
             "grid4": dict(size=32, patch=8, B=4, seeds=list(range(6)), n_global=1, n_local=4, global_scale=(0.7, 1.0),
                           local_scale=(0.45, 0.6), overlap=False, min_keep=4)}
    for name, c in cases.items():
        enc = vtt.VTT(image_size=c["size"], tactile_size=32, image_patch_size=c["patch"], tactile_patch_size=8, dim=64, depth=1, heads=1,
                      mlp_dim=64, num_tactiles=2, num_register_tokens=1)
        model = vtd.VTDINO(encoder=enc, dino_head=partial(DINOHead, out_dim=64, hidden_dim=32, bottleneck_dim=16), optim_cfg=None,
                           lr_scheduler_cfg=None, wd_scheduler_cfg=None, local_mask_scale=c["local_scale"], global_mask_scale=c["global_scale"],
                           num_global_masks=c["n_global"], num_local_masks=c["n_local"], min_keep_num_sensors=c["min_keep"],
                           allow_mask_overlap=c["overlap"], teacher_temp=0.05)
        x = torch.zeros(c["B"], 3, c["size"], c["size"])
        out[name + "/cfg"] = np.array([c["size"], c["patch"], c["B"], c["n_global"], c["n_local"], int(c["overlap"]), c["min_keep"]])
        out[name + "/scales"] = np.array(list(c["global_scale"]) + list(c["local_scale"]), dtype=np.float64)
        out[name + "/seeds"] = np.array(c["seeds"])
        for seed in c["seeds"]:
            model.generator.manual_seed(seed)
            with time_limit(60, f"sample_masks {name} seed {seed}"):      # fails loudly: no seed is dropped
                gm, lm = model.sample_masks(x)
            for i, m in enumerate(gm):
                out[f"{name}/seed{seed}/global/{i}"] = m.numpy()
            for i, m in enumerate(lm):
                out[f"{name}/seed{seed}/local/{i}"] = m.numpy()
    np.savez_compressed(os.path.join(HERE, "vtdino_masks.npz"), **out)


# ---- fixture 3: head -----------------------------------------------------------------------------------------------------------------
def make_head(DINOHead):
    out = {}
    cfg = dict(in_dim=64, out_dim=256, hidden_dim=128, bottleneck_dim=32)
    out["cfg"] = np.array([cfg["in_dim"], cfg["out_dim"], cfg["hidden_dim"], cfg["bottleneck_dim"]])
    torch.manual_seed(5)
    head = DINOHead(**cfg)
    for k, v in head.state_dict().items():
        out["init3/" + k] = v.numpy().copy()
    torch.manual_seed(6)
    head1 = DINOHead(nlayers=1, mlp_bias=False, **cfg)
    for k, v in head1.state_dict().items():
        out["init1/" + k] = v.numpy().copy()
    g = torch.Generator().manual_seed(7)
    with torch.no_grad():
        head.last_layer.weight_g.add_(0.3 * torch.randn(head.last_layer.weight_g.shape, generator=g))
        for n_, p in head.named_parameters():
            if n_.endswith("bias"):
                p.add_(0.1 * torch.randn(p.shape, generator=g))
    for k, v in head.state_dict().items():
        out["param/" + k] = v.numpy().copy()
    x = torch.randn(6, cfg["in_dim"], generator=g)
    dy = torch.randn(6, cfg["out_dim"], generator=g)
    out["x"], out["dy"] = x.numpy(), dy.numpy()
    head = head.double()
    xd = x.double().requires_grad_(True)
    y = head(xd)
    y.backward(dy.double())
    out["y"], out["dx"] = y.detach().numpy(), xd.grad.numpy()
    for n_, p in head.named_parameters():
        out["grad/" + n_] = p.grad.numpy()
    np.savez_compressed(os.path.join(HERE, "dino_head_init.npz"), **out)


# ---- fixture 4: loss in float64 ------------------------------------------------------------------------------------------------------
def make_loss(DINOLoss):
    P, Q, B, K = 3, 2, 3, 1000
    g = torch.Generator().manual_seed(11)
    loss_mod = DINOLoss(out_dim=K).double()
    loss_mod.center = (0.3 * torch.randn(1, K, generator=g)).double()
    out = {"dims": np.array([P, Q, B, K]), "student_temp": np.float64(loss_mod.student_temp), "center_momentum": np.float64(loss_mod.center_momentum),
           "center0": loss_mod.center.numpy().copy()}
    for call, tt in enumerate((0.04, 0.07)):
        S = (2.0 * torch.randn(P, B, K, generator=g)).double().requires_grad_(True)
        T = (2.0 * torch.randn(Q, B, K, generator=g)).double()
        probs = loss_mod.softmax_center_teacher(T.reshape(Q * B, K), teacher_temp=tt).view(Q, B, K)
        loss_mod.update_center(T.reshape(Q * B, K))
        loss = loss_mod(list(S.unsqueeze(2)), list(probs.unsqueeze(2)))
        loss.backward()
        pre = f"call{call}/"
        out[pre + "teacher_temp"] = np.float64(tt)
        out[pre + "S"], out[pre + "T"] = S.detach().numpy(), T.numpy()
        out[pre + "center_used"] = loss_mod.center.numpy().copy()
        out[pre + "probs"], out[pre + "loss"], out[pre + "dS"] = probs.numpy(), np.float64(loss.item()), S.grad.numpy()
        out[pre + "pending"] = loss_mod.async_batch_center.numpy().copy()
    loss_mod.apply_center_update()
    out["center_final"] = loss_mod.center.numpy().copy()
    np.savez_compressed(os.path.join(HERE, "dino_loss_f64.npz"), **out)


if __name__ == "__main__":
    vtt, vtd, DINOHead, DINOLoss = load_reference()
    make_loss(DINOLoss)
    make_head(DINOHead)
    make_masks(vtt, vtd, DINOHead)
    make_step(vtt, vtd, DINOHead)
    for f in sorted(os.listdir(HERE)):
        if f.startswith(("vtdino", "dino_head", "dino_loss")) and f.endswith(".npz"):
            print(f, os.path.getsize(os.path.join(HERE, f)))
