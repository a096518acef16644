"""Time of one DINO self-distillation step at the reference configuration (EXPERIMENTS.md "DINO step").

Encoder 256 wide / depth 4 / 8 heads / mlp 512 / one register token, 64x64 image at patch 8 and two 32x32 tactiles at patch 4, head
256 -> 2048 -> 2048 -> 256 -> 65536, 2 global + 8 local masks (local scale (0.2, 0.48): the reference's 0.1 lower bound can draw a block
that never passes), B = 32, in bf16 and in fp32.

  1. ms per step of the reference trainer's whole loop body (tactile_ssl/trainer/trainer.py:305-342): training_step + backward,
     clip_gradients(--grad-clip), AdamW over the two parameter groups, zero_grad, on_train_batch_end (teacher temperature, moving average),
     WarmupCosineScheduler and CosineWDSchedule.  --optimizer torch: clip_grad_norm_ + torch.optim.AdamW + the unfused moving average;
     --optimizer fused: m3l_amd.DinoAdamW(max_grad_norm) with the teacher bound (clip, update and average in three launches).  Mean over
     --steps steps after --warmup steps (CUDA events around the whole loop, one synchronisation at the end; training_step itself reads the
     loss back each step, as the reference's does).  Also: the host time spent enqueueing the tail (everything after the backward) per
     step, and the tail's device launches counted by torch's profiler in one further step.
  2. With the in-library event brackets (m3l_prof_*) on every launch for --prof-steps further steps: the share of the bracketed kernel
     time spent in head + loss (the new kernels and every GEMM / column sum over the register-token rows or the prototypes), and for each loss
     kernel its algorithmic bytes per launch and the rate they amount to against the 6.3 TB/s the HBM achieves.  The brackets serialise
     the launches, so (2) apportions time and (1) is the step time.

--centering sinkhorn_knopp runs the step with the Sinkhorn-Knopp teacher targets (three column passes and two extra row passes over the
64 x 65536 teacher logits per step, no centre update).  --koleo-weight W runs it with VTDINO(koleo_weight=W): the KoLeo regulariser over the
two global views' register rows (2 groups of 32 rows of 256), 3 + 1 launches per step.  --ibot runs it with VTDINO(ibot=True): the iBOT patch loss
over the 2 x (32 x 3 n) patch rows of the global views (n = 25 to 64 patches of the 8 x 8 grid per modality at this global scale), through
`dino_head` or, with --ibot-separate-head, a head of its own.  Every run also reports the peak device memory of the timed steps, so a run with and
one without --ibot in the same job give the term's cost in time and memory.

There is no pass mark.  Usage: python tools/bench_dino.py [--optimizer torch|fused] [--grad-clip 10.0] [--centering sinkhorn_knopp]
[--koleo-weight 0.1] [--ibot [--ibot-separate-head]]   (one JSON line on stdout)"""
import argparse
import ctypes as C
import json
import os
import sys
import time
from functools import partial

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import m3l_amd  # noqa: E402
from m3l_amd import _lib as L  # noqa: E402

DEV = "cuda:0"
HBM_TBS = 6.3
B, N_GLOBAL, N_LOCAL, K_OUT = 32, 2, 8, 65536
NEW_KINDS = ("dino_", "sk_", "koleo_", "ibot_", "l2norm", "weightnorm", "ema")      # ("dino_" covers dino_opt, the fused update launch)


def build(dt, centering="centering", koleo_weight=0.0, ibot=False, ibot_separate_head=False, optimizer="torch", grad_clip=10.0):
    torch.manual_seed(0)
    enc = m3l_amd.DinoVTT(image_size=64, tactile_size=32, image_patch_size=8, tactile_patch_size=4, dim=256, depth=4, heads=8, mlp_dim=512,
                          num_tactiles=2, num_register_tokens=1, compute_dtype=dt)
    clip = grad_clip if grad_clip > 0 else None
    optim_cfg = (partial(m3l_amd.DinoAdamW, lr=5e-4, weight_decay=0.05, max_grad_norm=clip) if optimizer == "fused"
                 else partial(torch.optim.AdamW, lr=5e-4, weight_decay=0.05))
    model = m3l_amd.VTDINO(encoder=enc, dino_head=partial(m3l_amd.DINOHead, out_dim=K_OUT, use_bn=False, nlayers=3, hidden_dim=2048, bottleneck_dim=256),
                           optim_cfg=optim_cfg,
                           lr_scheduler_cfg=partial(m3l_amd.WarmupCosineScheduler, start_lr=1e-5, warmup_epochs=1, final_lr=1e-6),
                           wd_scheduler_cfg=partial(m3l_amd.CosineWDSchedule, ref_weight_decay=0.05, final_weight_decay=0.4),
                           local_mask_scale=(0.2, 0.48), global_mask_scale=(0.48, 1.0), num_global_masks=N_GLOBAL, num_local_masks=N_LOCAL,
                           min_keep_num_sensors=4, allow_mask_overlap=True, moving_average_decay=[0.994, 1.0], teacher_temp=[0.04, 0.07],
                           **({} if centering == "centering" else {"centering": centering}),
                           **({"koleo_weight": koleo_weight} if koleo_weight else {}),
                           **({"ibot": True, "ibot_separate_head": ibot_separate_head} if ibot else {})).to(DEV)
    opt, lr_entry, wd_entry = model.configure_optimizers(100, 10)
    model.lr_scheduler, model.wd_scheduler = lr_entry["scheduler"], wd_entry["wd_scheduler"]
    if optimizer == "fused":
        opt.bind_teacher(model)
    model.grad_clip = clip
    model.clip_params = None if optimizer == "fused" or clip is None else [p for p in model.parameters() if p.requires_grad]
    model.tail_s = 0.0              # host time spent enqueueing the iteration tail (everything after the backward)
    g = torch.Generator().manual_seed(1)
    x = {"image": torch.rand(B, 3, 64, 64, generator=g).to(DEV), "tactile1": torch.rand(B, 3, 32, 32, generator=g).to(DEV),
         "tactile2": torch.rand(B, 3, 32, 32, generator=g).to(DEV)}
    return model, opt, x


def step(model, opt, x, i):
    """The reference trainer's loop body (tactile_ssl/trainer/trainer.py:305-342): training_step + backward, clip_gradients, optimizer.step(),
    zero_grad(), on_train_batch_end (teacher temperature, moving average), lr scheduler, wd scheduler."""
    out = model.training_step(x, i)
    out["loss"].backward()
    t0 = time.perf_counter()
    if model.clip_params is not None:
        torch.nn.utils.clip_grad_norm_(model.clip_params, model.grad_clip)
    opt.step()
    opt.zero_grad()
    model.on_train_batch_end(out, x, i)
    model.lr_scheduler.step()
    model.wd_scheduler.step()
    model.tail_s += time.perf_counter() - t0
    return out["ssl_loss"]


def tail_kernels(model, opt, x, i):
    """Device launches of one iteration tail, counted by torch's profiler (kernels and memsets after the backward)."""
    from torch.profiler import ProfilerActivity, profile
    out = model.training_step(x, i)
    out["loss"].backward()
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        if model.clip_params is not None:
            torch.nn.utils.clip_grad_norm_(model.clip_params, model.grad_clip)
        opt.step()
        opt.zero_grad()
        model.on_train_batch_end(out, x, i)
        model.lr_scheduler.step()
        model.wd_scheduler.step()
        torch.cuda.synchronize()
    return sum(e.count for e in prof.key_averages() if getattr(e, "device_time_total", 0) > 0)


def is_head(name):
    kind, dims = name.split("[")
    dims = [int(d) for d in dims.rstrip("]").split("x")]
    rows = {(N_GLOBAL + N_LOCAL) * B, N_GLOBAL * B}
    # a head launch has the P B or Q B rows of the register tokens as its M, or the prototype count among its dimensions (the encoder's
    # launches have thousands of token rows as M); the optimizer's launch is listed with the new kernels but is no head launch
    if kind.startswith("dino_opt"):
        return False
    return kind.startswith(NEW_KINDS) or K_OUT in dims or (kind.startswith(("gemm", "wgrad", "colsum")) and dims[0] in rows)


def classes():
    lib = L.lib()
    out = {}
    for i in range(lib.m3l_prof_count()):
        name = C.create_string_buffer(96)
        ms, n, w, b = C.c_double(), C.c_long(), C.c_double(), C.c_double()
        lib.m3l_prof_get(i, name, 96, C.byref(ms), C.byref(n), C.byref(w), C.byref(b))
        if n.value:
            out[name.value.decode()] = (ms.value, n.value, b.value)
    return out


def run(dt, steps, warmup, prof_steps, centering="centering", koleo_weight=0.0, ibot=False, ibot_separate_head=False, optimizer="torch", grad_clip=10.0):
    model, opt, x = build(dt, centering, koleo_weight, ibot, ibot_separate_head, optimizer, grad_clip)
    for i in range(warmup):
        loss = step(model, opt, x, i)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    model.tail_s = 0.0
    e0.record()
    for i in range(warmup, warmup + steps):
        loss = step(model, opt, x, i)
    e1.record()
    torch.cuda.synchronize()
    res = {"ms_per_step": round(e0.elapsed_time(e1) / steps, 3), "loss_last": round(loss, 4),
           "peak_memory_mb": round(torch.cuda.max_memory_allocated() / 2 ** 20, 1), "tail_host_us_per_step": round(model.tail_s / steps * 1e6, 1)}
    try:
        res["tail_launches"] = tail_kernels(model, opt, x, warmup + steps)
    except Exception as e:      # noqa: BLE001  (a build of torch without the device profiler: the count is left out)
        res["tail_launches"] = f"unavailable: {type(e).__name__}"
    L.lib().m3l_prof_begin(None, 1)
    for i in range(prof_steps):
        step(model, opt, x, warmup + steps + 1 + i)
    torch.cuda.synchronize()
    L.lib().m3l_prof_end()
    cls = classes()
    total = sum(v[0] for v in cls.values())
    head = sum(v[0] for k, v in cls.items() if is_head(k))
    res["bracketed_kernel_ms_per_step"] = round(total / prof_steps, 3)
    res["head_loss_ms_per_step"] = round(head / prof_steps, 3)
    res["head_loss_share"] = round(head / total, 3) if total else None
    res["new_kernels"] = {k: {"us_per_launch": round(v[0] / v[1] * 1e3, 1), "launches_per_step": v[1] / prof_steps,
                              "mb_per_launch": round(v[2] / v[1] / 1e6, 2), "tb_per_s": round(v[2] / v[0] / 1e9, 3),
                              "of_hbm_rate": round(v[2] / v[0] / 1e9 / HBM_TBS, 3)}
                          for k, v in sorted(cls.items()) if k.startswith(NEW_KINDS)}
    res["head_gemms"] = {k: {"us_per_launch": round(v[0] / v[1] * 1e3, 1), "launches_per_step": v[1] / prof_steps}
                         for k, v in sorted(cls.items()) if is_head(k) and not k.startswith(NEW_KINDS)}
    res["loss_kernel_mb_per_step"] = round(sum(v[2] for k, v in cls.items() if k.startswith(("dino_", "ibot_"))) / prof_steps / 1e6, 1)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--prof-steps", type=int, default=3)
    ap.add_argument("--dtypes", default="bf16,fp32")
    ap.add_argument("--centering", default="centering", choices=["centering", "sinkhorn_knopp"], help="teacher targets (VTDINO's keyword)")
    ap.add_argument("--koleo-weight", type=float, default=0.0, help="VTDINO's koleo_weight (0 = the step without the regulariser)")
    ap.add_argument("--ibot", action="store_true", help="VTDINO(ibot=True): add the iBOT patch loss")
    ap.add_argument("--ibot-separate-head", action="store_true", help="with --ibot: VTDINO(ibot_separate_head=True)")
    ap.add_argument("--optimizer", default="torch", choices=["torch", "fused"],
                    help="torch: clip_grad_norm_ + torch.optim.AdamW + the unfused moving average; fused: DinoAdamW with the teacher bound")
    ap.add_argument("--grad-clip", type=float, default=10.0, help="max gradient norm (the reference trainer's 10.0); 0 = no clipping")
    a = ap.parse_args()
    if a.ibot_separate_head and not a.ibot:
        ap.error("--ibot-separate-head needs --ibot")
    out = {"config": f"DinoVTT 256/4/8/512 + head 256-2048-2048-256-{K_OUT}, B={B}, {N_GLOBAL}+{N_LOCAL} views", "hbm_tb_per_s": HBM_TBS,
           "centering": a.centering, "koleo_weight": a.koleo_weight, "ibot": a.ibot, "ibot_separate_head": a.ibot_separate_head,
           "optimizer": a.optimizer, "grad_clip": a.grad_clip}
    for dt in a.dtypes.split(","):
        out[dt] = run(dt, a.steps, a.warmup, a.prof_steps, a.centering, a.koleo_weight, a.ibot, a.ibot_separate_head, a.optimizer, a.grad_clip)
        torch.cuda.empty_cache()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
