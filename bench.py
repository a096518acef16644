#!/usr/bin/env python3
"""Headline benchmark: MAE fwd+bwd samples/s (image + tactile) on N x MI355X — BASELINE.json configs[1] per GPU
(VTT vision+tactile MAE: 64x64 RGB + 2x32x32 tactile, ViT-Tiny 192/12/3/768, decoder 192/4/3/768, mask 75 %,
batch 256 per GPU, bf16 compute), synthetic random frames, random-init weights.

One "step" = zero_grad + mask sampling + VTMAE forward + backward (+ RCCL gradient all-reduce when N > 1)
+ Adam(lr=1e-4) update (reference: models/ppo_mae.py:182-183,262-266; the update runs as ONE HIP launch over the flat
parameter buffer, m3l_amd.parallel.FlatAdam, numerically torch.optim.Adam).  Weak scaling: 256 samples per GPU.

  python bench.py --gpus 1 --steps 20 --warmup 5
  python bench.py --gpus 1 --steps 20 --warmup 5 --dump-outputs bench_outputs   # + the last timed step's outputs as <DIR>/<name>.npy
  python bench.py --full                                                # + every figure beyond the headline (below)
  python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1 --master-port P bench.py --gpus N ...

Rank 0 prints ONE JSON line: the headline `value` (samples/s) and `ms_per_step` of the K timed steps.  With --full the timed region
also carries HIP-event brackets around the dominant kernel, and the line adds `roofline` (that kernel), `kernel_ms_sampled`, figures
quoted from profiles/, `secondary` (other architectures, timed after the headline run) and `cpu_baseline` (the CPU oracle timed on the
host's cores on a bounded sample).
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import torch  # noqa: E402
import torch.distributed as dist  # noqa: E402

PEAK_BF16_TFLOPS = 2500.0     # dense bf16 MFMA peak of MI355X (/opt/skills/guides/MI355X_MICROARCH.md)

CFG2 = dict(image_size=64, tactile_size=32, image_patch_size=8, tactile_patch_size=4, dim=192, depth=12, heads=3, mlp_dim=768,
            dec_dim=192, dec_depth=4, dec_heads=3, ratio=0.75, num_tactiles=2)


# BASELINE configs[3] (224x224 + 4x64x64, ViT-Small encoder, 4-layer decoder; sizes fixed by SURVEY.md section 8): selectable with
# --workload cfg4 for the multi-GPU ViT-Small measurement; the headline line (no flag) is always configs[1]
CFG4 = dict(image_size=224, tactile_size=64, image_patch_size=16, tactile_patch_size=8, dim=384, depth=12, heads=6, mlp_dim=1536,
            dec_dim=192, dec_depth=4, dec_heads=3, ratio=0.75, num_tactiles=4)
# BASELINE configs[4]'s MAE (train_dino_cat_mae.py:76,78,138-160: 70x70 frames, P = 14, frame_stack 4 -> 12 channels, 384/4/4/768, decoder
# 384/3/4, mask 0.8) and M3L's own default architecture (train.py:58-67,128-153: 256/4/4/512, decoder 256/3/4, early_conv_masking=True,
# frame_stack 4, mask 0.95): not headline workloads — timed briefly after the headline run and reported under "secondary"
CFG5 = dict(image_size=70, tactile_size=70, image_patch_size=14, tactile_patch_size=14, dim=384, depth=4, heads=4, mlp_dim=768,
            dec_dim=384, dec_depth=3, dec_heads=4, ratio=0.8, num_tactiles=2, channels=12, frame_stack=4)
CFGREF = dict(image_size=64, tactile_size=32, image_patch_size=8, tactile_patch_size=4, dim=256, depth=4, heads=4, mlp_dim=512,
              dec_dim=256, dec_depth=3, dec_heads=4, ratio=0.95, num_tactiles=2, channels=12, frame_stack=4, early_conv=True)
WORKLOADS = {
    "cfg2": (CFG2, 256, "BASELINE configs[1]: VTT vision+tactile MAE, 64x64 RGB + 2x32x32 tactile, ViT-Tiny 192/12/3/768 + decoder 192/4/3/768, mask 0.75"),
    "cfg4": (CFG4, 64, "BASELINE configs[3]: 224x224 RGB + 4x64x64 tactile, ViT-Small 384/12/6/1536 + decoder 192/4/3/768, mask 0.75"),
    "cfg5": (CFG5, 128, "BASELINE configs[4] MAE: 3 x 70x70 frames x frame_stack 4, P14, 384/4/4/768 + decoder 384/3/4/1536, mask 0.8"),
    "ref": (CFGREF, 512, "M3L default architecture (train.py:58-67,128-153): 256/4/4/512 + decoder 256/3/4/1024, EarlyCNN stems, frame_stack 4, mask 0.95"),
}


def fwd_flops_per_sample(c):
    """SURVEY.md section 8(d) formula (forward; fwd+bwd = 3x)."""
    def tf(n, D, depth, h, mlp):
        hd = h * 64
        return depth * (6 * n * D * hd + 4 * n * n * hd + 2 * n * hd * D + 4 * n * D * mlp)
    n_img, n_tac = (c["image_size"] // c["image_patch_size"]) ** 2, (c["tactile_size"] // c["tactile_patch_size"]) ** 2
    k = c["num_tactiles"]
    N = n_img + k * n_tac
    nmask = int(c["ratio"] * N)
    nm_img = int(nmask * (n_img / N))
    nm_tac = (nmask - nm_img) // k
    nvis = N - nm_img - k * nm_tac
    ch = c.get("channels", 3)
    pd_i, pd_t = ch * c["image_patch_size"] ** 2, ch * c["tactile_patch_size"] ** 2
    embed = 2 * (n_img - nm_img) * pd_i * c["dim"] + 2 * k * (n_tac - nm_tac) * pd_t * c["dim"]
    heads = 2 * nm_img * c["dec_dim"] * pd_i + 2 * k * nm_tac * c["dec_dim"] * pd_t
    if c.get("early_conv"):      # EarlyCNN stems over whole frames (pretrain_models.py:37-56) and the loss over ALL patches (:311-322)
        def stem(hw, tactile):
            D, f, ci, tot = c["dim"], 0, ch, 0
            for l, co in enumerate((D // 8, D // 4, D // 2, D)):
                kh, st_, pad = (1, 1, 0) if l == 3 else ((3, 1, 1) if (l == 2 and tactile) else (4, 2, 1))
                hw = (hw + 2 * pad - kh) // st_ + 1
                tot += 2 * hw * hw * ci * kh * kh * co
                ci = co
            return tot
        embed = stem(c["image_size"], False) + k * stem(c["tactile_size"], True)
        heads = 2 * n_img * c["dec_dim"] * pd_i + 2 * k * n_tac * c["dec_dim"] * pd_t
    return embed + tf(nvis, c["dim"], c["depth"], c["heads"], c["mlp_dim"]) + tf(N, c["dec_dim"], c["dec_depth"], c["dec_heads"], 4 * c["dec_dim"]) + heads


def attn_gemm_fwd_flops_per_sample(c):
    """QK^T + AV of every layer, forward (4 n^2 h d_h per layer)."""
    n_img, n_tac = (c["image_size"] // c["image_patch_size"]) ** 2, (c["tactile_size"] // c["tactile_patch_size"]) ** 2
    k = c["num_tactiles"]
    N = n_img + k * n_tac
    nmask = int(c["ratio"] * N)
    nm_img = int(nmask * (n_img / N))
    nvis = N - nm_img - k * ((nmask - nm_img) // k)
    return c["depth"] * 4 * nvis * nvis * c["heads"] * 64 + c["dec_depth"] * 4 * N * N * c["dec_heads"] * 64


def build_model(c, dtype, device):
    from m3l_amd import VTMAE, VTT
    torch.manual_seed(0)
    ch, fs = c.get("channels", 3), c.get("frame_stack", 1)
    enc = VTT(image_size=c["image_size"], tactile_size=c["tactile_size"], image_patch_size=c["image_patch_size"],
              tactile_patch_size=c["tactile_patch_size"], dim=c["dim"], depth=c["depth"], heads=c["heads"], mlp_dim=c["mlp_dim"],
              num_tactiles=c["num_tactiles"], image_channels=ch, tactile_channels=ch, frame_stack=fs)
    mae = VTMAE(encoder=enc, decoder_dim=c["dec_dim"], masking_ratio=c["ratio"], decoder_depth=c["dec_depth"],
                decoder_heads=c["dec_heads"], num_tactiles=c["num_tactiles"], compute_dtype=dtype,
                early_conv_masking=c.get("early_conv", False), frame_stack=fs)
    return mae.to(device)


def synthetic_batch(c, B, device, generator=None):
    ch = c.get("channels", 3)
    x = {"image": torch.rand(B, ch, c["image_size"], c["image_size"], device=device, generator=generator)}
    for i in range(c["num_tactiles"]):
        x[f"tactile{i + 1}"] = torch.rand(B, ch, c["tactile_size"], c["tactile_size"], device=device, generator=generator)
    return x


def secondary_workloads(dtype, dev, names=("cfg4", "cfg5", "ref"), steps=10, warmup=5):
    """Short driver-timed runs of the other architectures (same step: zero_grad + mask + fwd + bwd + Adam), one GPU, after the headline
    measurement: samples/s and ms/step each.  They make DESIGN.md section 5's secondary figures checkable in the driver's own run."""
    from m3l_amd.parallel import FlatAdam, GradSync
    rows = {}
    for name in names:
        c, B, desc = WORKLOADS[name]
        mae = build_model(c, dtype, dev)
        sync = GradSync(mae)
        opt = FlatAdam(sync, lr=1e-4)
        x = synthetic_batch(c, B, dev)

        def step():
            sync.zero_grad()
            loss = mae(x)
            loss.backward()
            sync.finish(defer_scale=True)
            opt.step()
            return loss
        for _ in range(warmup):
            step()
        # three windows of `steps` steps, the median one reported: a single host / allocator hiccup of a few tens of ms inside a 20-60 ms
        # window otherwise halves a figure (seen once in a while on the pool's boxes; the headline measurement keeps the contract's
        # single K-step window)
        els, enq = [], []
        for _ in range(3):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(steps):
                loss = step()
            enq.append(time.perf_counter() - t0)
            torch.cuda.synchronize()
            els.append(time.perf_counter() - t0)
        el = sorted(els)[1]
        rows[name] = {"workload": desc, "batch": B, "steps": steps, "windows": 3, "ms_per_step": round(el / steps * 1e3, 3),
                      "samples_per_s": round(B * steps / el, 1), "model_tflops": round(3 * fwd_flops_per_sample(c) * B * steps / el / 1e12, 1),
                      "host_enqueue_ms_per_step": round(sorted(enq)[1] / steps * 1e3, 3), "loss": round(float(loss.detach()), 5)}
        if name == "ref":
            rows.update(extractor_rows(mae, c, dev, steps, warmup))
        del mae, sync, opt, x
        torch.cuda.empty_cache()
    return rows


def extractor_rows(mae, c, dev, steps, warmup):
    """the policy-side consumer of the MAE, `MAEExtractor.forward` (models/pretrain_models.py:819-841) on M3L's default
    architecture — observations -> vt_load -> get_embeddings over all tokens -> the extractor's 1-layer Transformer -> mean — as the
    reference calls it: on every environment step at B = 8 under no_grad (a latency figure: obs/s and ms per call) and on every PPO
    minibatch at B = 512 with grad (models/ppo_mae.py:280; forward + backward, samples/s).  Both through m3l_extractor_fwd / _bwd."""
    from m3l_amd import MAEExtractor
    fs = c.get("frame_stack", 1)
    ext = MAEExtractor(mae, c["dim"], False, fs).to(dev)
    out = {}
    for tag, B, grad in (("extractor_rollout_B8", 8, False), ("extractor_train_B512", 512, True)):
        obs = {"image": torch.rand(B, fs, c["image_size"], c["image_size"], 3, device=dev),
               "tactile": torch.rand(B, fs, 3 * c["num_tactiles"], c["tactile_size"], c["tactile_size"], device=dev) * 2 - 1}

        def call():
            if not grad:
                with torch.no_grad():
                    return ext(obs)
            ext.zero_grad(set_to_none=True)
            f = ext(obs)
            f.square().mean().backward()
            return f
        for _ in range(warmup):
            call()
        els = []
        for _ in range(3):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(steps):
                call()
            torch.cuda.synchronize()
            els.append(time.perf_counter() - t0)
        el = sorted(els)[1]
        out[tag] = {"workload": ("MAEExtractor.forward under no_grad (rollout)" if not grad else "MAEExtractor forward + backward (PPO minibatch)") +
                                " on the M3L default architecture, vt_load included", "batch": B, "steps": steps, "windows": 3,
                    "ms_per_call": round(el / steps * 1e3, 3), "obs_per_s": round(B * steps / el, 1)}
    return out


CFG1 = dict(CFG2, num_tactiles=0)     # BASELINE configs[0]: vision-only MAE, 64x64 RGB, ViT-Tiny, mask 75 %, batch 8 on CPU


def _socket_cores():
    """Physical cores of one socket that this process may use (cgroup / affinity aware)."""
    allowed = len(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else (os.cpu_count() or 1)
    try:
        cores = set()
        phys = core = None
        for line in open("/proc/cpuinfo"):
            if line.startswith("physical id"):
                phys = int(line.split(":")[1])
            elif line.startswith("core id"):
                core = int(line.split(":")[1])
            elif not line.strip():
                if phys == 0 and core is not None:
                    cores.add(core)
                phys = core = None
        n = len(cores) or allowed
    except OSError:
        n = allowed
    return max(1, min(n, allowed))


def _cpu_measure(c, B, threads, warmups, iters, cap_s):
    """Median samples/s of the CPU oracle (fwd + bwd, fp32) on architecture c at batch B with `threads` torch threads: `warmups` untimed
    iterations, then up to `iters` timed ones or until `cap_s` seconds have been spent (at least one)."""
    from oracle import vtmae_oracle as O
    torch.set_num_threads(threads)
    torch.manual_seed(0)
    mae = build_model(c, "fp32", "cpu")
    P = {k: v.detach().clone().requires_grad_(v.dtype.is_floating_point) for k, v in mae.state_dict().items()}
    cfg = O.OracleCfg(c["image_size"], c["tactile_size"], c["image_patch_size"], c["tactile_patch_size"], c["dim"], c["depth"],
                      c["heads"], c["mlp_dim"], 3, c["num_tactiles"], c["dec_dim"], c["dec_depth"], c["dec_heads"], c["ratio"])
    g = torch.Generator().manual_seed(1234)
    x = {"image": torch.rand(B, 3, c["image_size"], c["image_size"], generator=g)}
    for i in range(c["num_tactiles"]):
        x[f"tactile{i + 1}"] = torch.rand(B, 3, c["tactile_size"], c["tactile_size"], generator=g)
    n_img, n_tac = (c["image_size"] // c["image_patch_size"]) ** 2, (c["tactile_size"] // c["tactile_patch_size"]) ** 2

    def step():
        noises = [torch.rand(B, n_img, generator=g)] + [torch.rand(B, n_tac, generator=g) for _ in range(c["num_tactiles"])]
        for p in P.values():
            p.grad = None
        O.vtmae_forward(P, cfg, x, noises)["loss"].backward()
    t_all = time.perf_counter()
    for _ in range(warmups):
        step()
        if time.perf_counter() - t_all > cap_s:        # a very slow configuration: do not spend the whole cap warming up
            break
    times = []
    t_all = time.perf_counter()
    while len(times) < iters and (not times or time.perf_counter() - t_all < cap_s):
        t0 = time.perf_counter()
        step()
        times.append(time.perf_counter() - t0)
    times.sort()
    med = times[len(times) // 2]
    return {"samples_per_s": round(B / med, 2), "batch": B, "threads": threads, "iters": len(times), "median_s": round(med, 4)}


def cpu_baseline():
    """BASELINE.md section 5 / SURVEY.md 8(d): the CPU oracle (a restatement of the reference's PyTorch path, fixture-verified) on this
    box's host cores — cfg 1 exactly (vision-only, B = 8) and cfg 2 at B = 64, each with 1 thread and with the physical cores of one
    socket; 5 warm-ups, median of up to 20 iterations, every measurement capped so that the whole baseline stays within ~35 s."""
    keep = torch.get_num_threads()
    sock = _socket_cores()
    rows = {}
    try:
        rows["cfg1_B8_1thread"] = _cpu_measure(CFG1, 8, 1, 5, 20, 5.0)
        rows["cfg1_B8_socket"] = _cpu_measure(CFG1, 8, sock, 5, 20, 4.0)
        rows["cfg2_B64_socket"] = _cpu_measure(CFG2, 64, sock, 5, 20, 14.0)
        rows["cfg2_B8_1thread"] = _cpu_measure(CFG2, 8, 1, 2, 20, 8.0)      # B = 64 on one thread is ~1 minute per iteration: B = 8 stated
    finally:
        torch.set_num_threads(keep)
    main = rows["cfg2_B64_socket"]
    cpu_model = ""
    try:
        cpu_model = next(line.split(":", 1)[1].strip() for line in open("/proc/cpuinfo") if line.startswith("model name"))
    except (OSError, StopIteration):
        pass
    return {"value": main["samples_per_s"], "unit": "samples/s", "cores": main["threads"], "kind": "port",
            "sample": f"CPU oracle (oracle/vtmae_oracle.py, torch {torch.__version__} fp32 + autograd), cfg-2 model at B=64 on {main['threads']} "
                      f"threads (physical cores of one socket available to this process; {os.cpu_count()} logical CPUs, {cpu_model}): "
                      f"median of {main['iters']} fwd+bwd iterations after 5 warm-ups, time-capped",
            "all": rows}


# --dump-outputs caps, in elements per array: cfg 2's parameters and gradients (7.2 M each) are written whole, and no dump exceeds
# 2 x 7.4 M + 2 x 0.5 M float32 values (under 64 MB)
DUMP_FLAT_CAP = 7_400_000
DUMP_MASK_CAP = 500_000


def _dump_array(t, cap):
    """t as float32 on the host; a tensor of more than `cap` elements is flattened and sampled at `cap` fixed indices (seeded: the same
    indices for the same size, so that two runs compare element for element)."""
    import numpy as np
    t = t.detach()
    if t.numel() > cap:
        idx = np.sort(np.random.default_rng(0).choice(t.numel(), cap, replace=False))
        t = t.reshape(-1)[torch.from_numpy(idx).to(t.device)]
    return t.float().cpu().numpy()


def dump_outputs(d, loss, last_mask, sync):
    """What the timed step hands its caller, from the last timed step: the loss, the masked / unmasked token indices (exact in float32),
    the gradients and the parameters after the Adam update (GradSync's flat buffers, in their order), as d/<name>.npy."""
    import numpy as np
    os.makedirs(d, exist_ok=True)
    arrays = {"loss": np.asarray([float(loss.detach())], dtype=np.float64),
              "masked_indices": _dump_array(last_mask[0], DUMP_MASK_CAP), "unmasked_indices": _dump_array(last_mask[1], DUMP_MASK_CAP),
              "grads": _dump_array(sync.flat, DUMP_FLAT_CAP), "params": _dump_array(sync.flat_params, DUMP_FLAT_CAP)}
    for name, a in arrays.items():
        np.save(os.path.join(d, name + ".npy"), a)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--workload", default="cfg2", choices=sorted(WORKLOADS), help="cfg2 = the headline metric (default); cfg4 = ViT-Small")
    ap.add_argument("--batch", type=int, default=0, help="samples per GPU (weak scaling); 0 = the workload's default (256 for cfg2)")
    ap.add_argument("--dtype", default="bf16", choices=["bf16", "fp32"])
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--no-secondary", action="store_true", help="skip the short secondary-workload runs (cfg 4, cfg 5 MAE, reference default)")
    ap.add_argument("--roofline-kernel", default="wgrad[", help="kernel class event-timed inside the timed region ('' = every tracked class, diagnostic)")
    ap.add_argument("--no-optimizer", action="store_true", help="diagnostic only: time fwd+bwd without the Adam update")
    ap.add_argument("--full", action="store_true", help="also measure everything beyond the headline line: roofline (event brackets inside the "
                                                        "timed region), profile figures, secondary workloads, CPU baseline")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="write the last timed step's loss, mask indices, gradients and updated parameters as DIR/<name>.npy")
    args = ap.parse_args()
    if args.steps < 1:
        ap.error("--steps must be at least 1")
    # stdout carries exactly ONE line, the result: anything else a library prints there (RCCL's version banner goes to stdout)
    # is sent to stderr by pointing fd 1 at fd 2 for the whole run and keeping the real stdout aside for the JSON line
    sys.stdout.flush()
    result_fd = os.dup(1)
    os.dup2(2, 1)

    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local = int(os.environ.get("LOCAL_RANK", "0"))
    if args.gpus > 1 and world != args.gpus:
        sys.exit(f"--gpus {args.gpus} needs torch.distributed.run with --nproc-per-node {args.gpus} (WORLD_SIZE={world})")
    # rehearsal of the N > 1 control flow on a box with fewer GPUs than ranks (ranks share devices, collectives go through gloo):
    # M3L_BENCH_REHEARSE=1.  Never used for a reported number.
    rehearse = os.environ.get("M3L_BENCH_REHEARSE") == "1"
    if rehearse:
        local = local % max(1, torch.cuda.device_count())
    torch.cuda.set_device(local)
    dev = torch.device("cuda", local)
    force_comm = os.environ.get("M3L_FORCE_COMM") == "1"       # rehearsal: RCCL calls at world size 1 (one-GPU box)
    if world > 1 or force_comm or os.environ.get("M3L_FORCE_COMM") == "2":      # "2": process group only (diagnostic)
        if "MASTER_ADDR" not in os.environ:
            os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT="29531", RANK="0", WORLD_SIZE="1")
        # (the gradient all-reduce does not use torch.distributed's NCCL stream at all: m3l_amd.parallel.GradSync has the library call RCCL
        # on its own side stream — a third kernel-bearing stream costs 7 % of the step at normal priority and 48 % at high priority, so
        # TORCH_NCCL_HIGH_PRIORITY must stay unset for the fallback path too)
        if rehearse:
            dist.init_process_group("gloo")
        else:
            dist.init_process_group("nccl", device_id=dev)

    from m3l_amd import _lib
    from m3l_amd.parallel import FlatAdam, GradSync
    _lib.lib()
    c, default_batch, workload_name = WORKLOADS[args.workload]
    if args.batch <= 0:
        args.batch = default_batch
    mae = build_model(c, args.dtype, dev)
    sync = GradSync(mae, force_comm=force_comm)
    opt = FlatAdam(sync, lr=1e-4)                 # torch.optim.Adam semantics, one HIP launch over the flat buffers
    B = args.batch
    init_params = sync.flat_params.clone()
    torch.manual_seed(1234 + rank)
    x = synthetic_batch(c, B, dev)

    def step():
        sync.zero_grad()
        loss = mae(x)                 # mask noise drawn on the device with torch.rand, as the reference does
        loss.backward()
        sync.finish(defer_scale=not args.no_optimizer)     # the 1 / world of the SUM all-reduce is folded into the Adam launch
        if not args.no_optimizer:
            opt.step()
        return loss

    def barrier():
        if dist.is_initialized():
            dist.barrier()
        torch.cuda.synchronize()

    # priming, always (not part of W or K): code-object load, allocator growth, side stream / event pool creation, and
    # ~2 s of back-to-back steps so that the clocks of a freshly booted box have settled before anything is timed
    t_prime = time.perf_counter()
    while True:
        for _ in range(5):
            step()
        torch.cuda.synchronize()
        done = time.perf_counter() - t_prime > 2.0
        if dist.is_initialized():                 # every rank must run the SAME number of steps (each step issues collectives)
            flag = torch.tensor([1.0 if done else 0.0], device=dev)
            dist.all_reduce(flag, op=dist.ReduceOp.MAX)
            done = bool(flag.item() > 0)
        if done:
            break
    # warm-up and timed steps start from the initial weights, fresh Adam moments and a fixed seed for the mask noise: the priming above
    # runs for a time, not a step count, so without this the last step's outputs (`loss`, --dump-outputs) would differ from run to run
    with torch.no_grad():
        sync.flat_params.copy_(init_params)
    del init_params
    opt.exp_avg.zero_()
    opt.exp_avg_sq.zero_()
    opt.step_count = 0
    torch.manual_seed(4321 + rank)
    for _ in range(args.warmup):
        step()
    lib = _lib.lib()
    barrier()
    if args.full:
        # launches of the roofline kernel are bracketed by HIP events on the stream they are launched on
        # (the weight-gradient class is 5-7 launches per step: every launch is bracketed — a stride that divides the per-step count would
        # sample the same launch of every step)
        prof_stride = 1 if (args.roofline_kernel or "").startswith("wgrad") else 5
        lib.m3l_prof_begin(args.roofline_kernel.encode() if args.roofline_kernel else None, prof_stride if args.roofline_kernel else 1)
    t0 = time.perf_counter()
    for _ in range(args.steps):
        loss = step()
    t_enq = time.perf_counter() - t0          # host done enqueueing (diagnostic: equal to `el` means the host is the bound)
    barrier()
    el = time.perf_counter() - t0
    if args.full:
        lib.m3l_prof_end()
        ev_overhead_us = lib.m3l_prof_event_overhead_us(torch.cuda.current_stream().cuda_stream, 200)
    if world > 1:
        t = torch.tensor([el], device=dev, dtype=torch.float64)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        el = float(t.item())
    ms = el / args.steps * 1e3
    value = B * world * args.steps / el
    if args.dump_outputs and rank == 0:
        dump_outputs(args.dump_outputs, loss, mae.last_mask, sync)

    out = {"metric": "MAE fwd+bwd samples/sec (image+tactile)", "value": round(value, 1), "unit": "samples/s",
           "n_gpus": world, "steps": args.steps, "warmup": args.warmup, "ms_per_step": round(ms, 3),
           "higher_is_better": True, "scaling": "weak", "vs_baseline": None, "dtype": args.dtype, "data": "synthetic",
           "config": {"workload": workload_name,
                      "batch_per_gpu": B, "global_batch": B * world, "parallelism": f"dp{world}",
                      "grad_allreduce": ("none (one rank)" if not sync._comm else
                                         "RCCL called by the library on its side stream" if getattr(sync, "_direct", False) else
                                         "torch.distributed (%s)" % dist.get_backend()),
                      "rccl_ranks": int(_lib.lib().m3l_comm_world()) if getattr(sync, "_direct", False) else 0,
                      "rccl_probe_sum": getattr(sync, "rccl_probe", None),     # all-reduce of (rank + 1) by the library's communicator = N (N + 1) / 2
                      "step": "zero_grad + mask + fwd + bwd + grad all-reduce + Adam" if not args.no_optimizer else "fwd + bwd (diagnostic)"},
           "loss": round(float(loss.detach()), 5), "host_enqueue_ms_per_step": round(t_enq / args.steps * 1e3, 3)}
    if rank == 0 and args.full:
        import ctypes as C
        # ---- roofline of the dominant kernel (HIP events recorded by the library around its launches, inside the timed region, on
        # the stream the kernel is launched on — the library's side stream for the weight gradients).  By rocprofv3
        # (profiles/r02_kernel_stats.csv) the single largest kernel of this step is the grouped weight-gradient GEMM
        # wgrad_kernel<3> (wgrad.hip): 288 FLOP per algorithmic byte at the decoder shapes, below 2500 TFLOP/s / 8 TB/s = 312, so
        # it is priced against the HBM roof; the MFMA rate it reaches is reported beside it.  Algorithmic bytes = both operands
        # once + dW once (the split-M slabs are implementation traffic and show up in `traffic`).
        def prof_kinds():
            kinds = {}
            for i in range(lib.m3l_prof_count()):
                name = C.create_string_buffer(96)
                ms_tot, launches, work, byt = C.c_double(), C.c_long(), C.c_double(), C.c_double()
                lib.m3l_prof_get(i, name, 96, C.byref(ms_tot), C.byref(launches), C.byref(work), C.byref(byt))
                if launches.value:
                    k = kinds.setdefault(name.value.decode().split("[")[0], [0.0, 0, 0.0, 0.0])
                    k[0] += ms_tot.value; k[1] += launches.value; k[2] += work.value; k[3] += byt.value
            return kinds

        kinds = prof_kinds()
        # The weight-gradient kernels run on the lowest-priority side stream and yield compute units to the critical path, so their
        # in-step launch duration (the `roofline` figure below, as the contract defines it) includes waiting.  Outside the timed region,
        # five more steps with every weight gradient on the compute stream (m3l_set_wgrad_inline) give the same kernel's duration when it
        # has the GPU to itself.
        kinds_alone = {}
        family = {}
        if world == 1 and args.roofline_kernel and kinds:
            old_inline = lib.m3l_set_wgrad_inline(1)
            for _ in range(3):
                step()
            barrier()
            lib.m3l_prof_begin(args.roofline_kernel.encode(), 1)
            for _ in range(5):
                step()
            barrier()
            lib.m3l_prof_end()
            kinds_alone = prof_kinds()
            # the whole weight-gradient family of a step (grouped launches, the small Linears' launches, the slab reduces): algorithmic
            # bytes and slab bytes per step, to set beside the counter bytes of the same launches (profiles/*_traffic.json)
            if args.roofline_kernel.startswith("wgrad"):
                lib.m3l_prof_begin(b"wgrad", 1)
                for _ in range(2):
                    step()
                barrier()
                lib.m3l_prof_end()
                family = {k: (v[1] / 2.0, v[3] / 2.0) for k, v in prof_kinds().items()}      # kind -> (launches, bytes) per step
            lib.m3l_set_wgrad_inline(old_inline)
        out["kernel_ms_sampled"] = {k: round(v[0] / args.steps, 4) for k, v in sorted(kinds.items(), key=lambda kv: -kv[1][0])}
        import glob
        prof_files = sorted(glob.glob(os.path.join(ROOT, "profiles", "r[0-9][0-9]_traffic.json")))
        prof_json = prof_files[-1] if prof_files else ""
        prof_name = os.path.join("profiles", os.path.basename(prof_json)) if prof_json else None
        prof = json.load(open(prof_json)) if prof_json else {}
        # what code the quoted profile was measured on, against what runs now (a stale profile must not feed a fresh
        # line silently): the profile tools copy m3l_amd/lib/build_stamp.json (git HEAD at build time + hash of the kernel sources) into
        # the files they write; this run recomputes the hash of the sources it was built from
        try:
            import __graft_entry__ as GE
            cur_sha = GE.sources_sha16()
        except Exception:      # noqa: BLE001  (diagnostic field only)
            cur_sha = None
        try:
            cur_stamp = json.load(open(os.path.join(ROOT, "m3l_amd", "lib", "build_stamp.json")))
        except (OSError, ValueError):
            cur_stamp = {}

        def prof_meta(p):
            m = p.get("_meta") or {}
            return {"profile_git_head": m.get("git_head"), "profile_git_dirty": m.get("git_dirty"), "profile_sources_sha16": m.get("sources_sha16"),
                    "run_sources_sha16": cur_sha, "run_git_head": cur_stamp.get("git_head") if cur_stamp.get("sources_sha16") == cur_sha else None,
                    "same_kernel_sources": (m.get("sources_sha16") == cur_sha) if (m.get("sources_sha16") and cur_sha) else None}
        if kinds:
            kname, (ms_tot, launches, work, byt) = max(kinds.items(), key=lambda kv: kv[1][0])
            raw_us = ms_tot / launches * 1e3
            avg_s = max(raw_us - ev_overhead_us, 0.1) * 1e-6       # bracket minus the empty-bracket cost = kernel time
            gbs = byt / launches / avg_s / 1e9
            kfull = {"wgrad": "wgrad_kernel<6,3> (384x192 tiles; the grouped per-layer launches)", "gemm_nt_glds64": "gemm_nt_glds_kernel<bf16,64,2,*>"}.get(kname, kname)
            traffic = prof.get("wgrad_grouped" if kname == "wgrad" else kname, prof.get(kname, {})).get("hbm_bytes_per_launch")
            out["roofline"] = {"kernel": kfull, "bound": "hbm", "achieved": round(gbs, 1), "peak": 8000.0, "unit": "GB/s",
                               "frac": round(gbs / 8000.0, 4), "traffic": traffic,
                               "traffic_profile": prof_meta(prof) if traffic else None,
                               "traffic_source": f"{prof_name}: rocprofv3 --pmc FETCH_SIZE / WRITE_SIZE passes of this command on the builder's GPU lease (not re-measured in this run), the same launch population as `achieved` (grouped launches only)" if traffic else None,
                               "algorithmic_bytes_per_launch": round(byt / launches), "avg_launch_us": round(avg_s * 1e6, 2),
                               "avg_bracket_us_raw": round(raw_us, 2), "event_bracket_overhead_us": round(ev_overhead_us, 2),
                               "launches_sampled": launches, "launches_per_step": round(launches * prof_stride / args.steps, 1),
                               "stand_alone": None,
                               "mfma_tflops": round(work / launches / avg_s / 1e12, 1), "mfma_frac_of_2500": round(work / launches / avg_s / 2.5e15, 4)}
            if family:
                # per step, like for like: counter bytes of every weight-gradient launch (kernel + slab reduce) against their algorithmic bytes
                alg = sum(v[1] for k, v in family.items() if k in ("wgrad", "wgrad_small"))
                slabs = sum(v[1] for k, v in family.items() if k == "wgrad_reduce")
                fam = prof.get("wgrad_family_per_step", {})
                pmc = fam.get("hbm_bytes_per_step")
                out["roofline"]["per_step"] = {
                    "launches": {k: v[0] for k, v in family.items()}, "algorithmic_bytes": round(alg), "split_m_slab_bytes": round(slabs),
                    "pmc_bytes": pmc, "pmc_over_algorithmic": round(pmc / alg, 3) if pmc and alg else None,
                    "note": "operands once + dW once (algorithmic) vs FETCH/WRITE counters of the same launches; the excess is the split-M slabs "
                            "(written once, read once by the reduce kernels) and operand rows staged by more than one column tile"}
            if kname in kinds_alone:
                a_ms, a_n, a_work, a_byt = kinds_alone[kname]
                a_s = max(a_ms / a_n * 1e3 - ev_overhead_us, 0.1) * 1e-6
                out["roofline"]["stand_alone"] = {
                    "note": "same kernel with the GPU to itself (5 extra steps after the timed region, weight gradients on the compute stream)",
                    "avg_launch_us": round(a_s * 1e6, 2), "achieved": round(a_byt / a_n / a_s / 1e9, 1), "frac": round(a_byt / a_n / a_s / 8e12, 4),
                    "launches_sampled": a_n, "mfma_tflops": round(a_work / a_n / a_s / 1e12, 1)}
        # whole-step HBM use: PMC bytes per step of the committed profile over THIS run's step time, and the three largest kernels of
        # the committed rocprofv3 trace with their own HBM fractions (so that the kernels furthest from the roof are visible)
        if prof.get("_step"):
            sb = prof["_step"]["hbm_bytes_per_step"]
            out["step_hbm"] = {"bytes_per_step": sb, "GBps": round(sb / (ms * 1e-3) / 1e9, 1), "frac_of_8TBps": round(sb / (ms * 1e-3) / 8e12, 4),
                               "source": f"{prof_name} (PMC, builder's lease) / this run's ms_per_step", "profile": prof_meta(prof)}
            out["top_kernels"] = prof["_step"].get("top_kernels")
        total_flops = 3 * fwd_flops_per_sample(c) * value
        out["model_tflops"] = round(total_flops / 1e12, 2)
        # BASELINE north_star: throughput also "as fraction of the attention-GEMM roofline" = QK^T + AV FLOPs (fwd + bwd = 3x fwd,
        # SURVEY 8d) at this sample rate over the dense bf16 MFMA peak of the GPUs used
        attn = 3 * attn_gemm_fwd_flops_per_sample(c) * value
        out["attention_gemm"] = {"tflops": round(attn / 1e12, 2), "frac_of_bf16_peak": round(attn / (world * PEAK_BF16_TFLOPS * 1e12), 5)}
        # BASELINE's ">= 40 % encoder-attention MFMA utilisation": measured per phase of the encoder's attention block by shader-clock
        # stamps (tools/attn_phase_probe.py -> profiles/rNN_attn_phases.json, builder's lease), with the bound this problem size allows
        ph_files = sorted(glob.glob(os.path.join(ROOT, "profiles", "r[0-9][0-9]_attn_phases.json")))
        if ph_files:
            ph = json.load(open(ph_files[-1]))
            out["encoder_attention_mfma"] = {
                "attention_phase_util": ph.get("phases", {}).get("attention", {}).get("mfma_util_issued"),
                "attention_phase_util_useful_keys": ph.get("phases", {}).get("attention", {}).get("mfma_util_useful"),
                "whole_attention_block_util": ph.get("kernel_mfma_util_useful"), "target": 0.40,
                "bound": "~0.27 at the HBM roof: one encoder layer is 4.1 GFLOP (256 samples x 48 visible tokens) = 1.6 us at the bf16 peak, and with every "
                         "activation saved for the backward the block moves ~86 FLOP per byte",
                "source": os.path.join("profiles", os.path.basename(ph_files[-1])) + " (in-kernel shader-clock stamps, not re-measured in this run)",
                "profile": prof_meta(ph)}
        if world == 1 and not args.no_secondary and args.workload == "cfg2":
            out["secondary"] = secondary_workloads(args.dtype, dev)
        if world == 1 and not args.no_cpu_baseline and args.workload == "cfg2":
            out["cpu_baseline"] = cpu_baseline()
    if rank == 0:
        os.write(result_fd, (json.dumps(out) + "\n").encode())
    if dist.is_initialized():
        sync.close()                      # the library's own RCCL communicator (collective), then torch's
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
