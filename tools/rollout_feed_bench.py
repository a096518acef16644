"""Time of getting one PPO minibatch to the MAE's input tensors (EXPERIMENTS.md §5.20), at PPO's shapes: a rollout of T = 4096 steps of
n_envs = 8 environments, frame_stack = 4, image 64 x 64 x 3, 2 tactile sensors at 32 x 32 x 3, minibatch B = 512; two store variants, uint8
image + float32 tactile (4.8 GB) and all float32 (9.7 GB).  Three paths, timed per minibatch:

  (a) host     what a user of the reference pays today (models/ppo_dino_cat_mae.py:48-56, :58-70, :295-301, :320): numpy fancy index into the
               swapped-and-flattened host rollout -> torch.as_tensor(...).to(device) from pageable memory -> _flatten_frame_stack -> vt_load
  (b) resident the same existing ops on a device-resident store: index_select -> _flatten_frame_stack -> vt_load.  The store is addressed by
               row numbers computed outside the timed region, which stands for a store swapped once per rollout, as `prepare()` does
  (c) gather   m3l_rollout_gather_load on the store as the vec-env filled it (m3l_amd.rollout.gather_load): one launch

Every call takes the next B indices of one fixed permutation of the 32768 rows, so no path re-reads rows the caches still hold.  Before the
timing the three paths' outputs for one minibatch are compared bit for bit: a wrong result cannot pass as a fast one.

Per path: call_us = device events around a window of back-to-back calls that ends in a synchronise (for (a) the device idles while the host
indexes, so the events span the host's work too); host_us = host clock around the same window without its synchronise.  The paths alternate
(a b c a b c ...), --rounds windows each; reported: the median window, minimum and maximum.  launches / copies per minibatch come from
torch.profiler over a few calls in a run of their own.  For (c): gbytes_per_s = the bytes the algorithm needs (one read of the sampled rows,
one write of the float32 result) over call_us, and its share of the 6.29 TB/s a float4 copy reaches on this chip (8.0 TB/s is the data-sheet
figure).  Without a GPU the tool fails; it has no fallback.

--shift / --dedup (EXPERIMENTS.md §5.30) time the read-side features of the same launch instead, on stores made on the device: a frame store
(T + fs - 1, n_envs, ...) of random frames with the ages of episodes of 20 to 400 steps, and the stacked store that the slot rule reads out of it, so both hold the same
observations and their batches are compared bit for bit before anything is timed.  In alternating windows of one run:
  stacked / stacked_parent   m3l_rollout_gather_load through this build and, with --parent-lib, through the parent commit's library; then
  / stacked_repeat           this build's once more, so that the place of a window in its round can be told from the build
  stacked_shift              m3l_rollout_gather_load_shift, pads --pads (default 4,2), shifts drawn once per batch outside the window   (--shift)
  frames / frames_shift      m3l_rollout_gather_load_frames[_shift] on the frame store                                                  (--dedup)
  torch_shift                the unshifted launch plus `torch_shift_baseline` on every tensor of the batch, with its launch count      (--shift)
and, outside the windows, one add() in both modes and store_bytes() at PPO's defaults.

Usage: python tools/rollout_feed_bench.py [--rounds 5] [--iters 200] [--host-iters 5] [--variants u8,f32] [--shift] [--dedup] [--pads 4,2]
       [--parent-lib PATH]   (one JSON line on stdout)"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import m3l_amd  # noqa: E402,F401
from m3l_amd import rollout as R  # noqa: E402
from m3l_amd import vt_load  # noqa: E402
from m3l_amd.fusion import _flatten_frame_stack  # noqa: E402

DEV = "cuda:0"
T, E, FS, H, W, S, TH, TW, B = 4096, 8, 4, 64, 64, 2, 32, 32, 512
HBM_COPY_TBS, HBM_SPEC_TBS = 6.29, 8.0


def torch_shift_baseline(x, shifts_b, pad):
    """The random shift from torch ops: x (B, C, H, W), shifts_b (B, 2) integers (dy, dx) -> out[b, c, y, x] = x[b, c, clamp(y + dy, 0, H - 1),
    clamp(x + dx, 0, W - 1)] with (dy, dx) clamped to [-pad, pad].  Every index is clamped to the pad and then to the frame before either
    torch.gather sees it: torch.gather does not check indices on the device.  tests/test_rollout_aug_cpu.py holds this function to the numpy
    definition on CPU tensors."""
    B, C, H, W = x.shape
    s = shifts_b.to(torch.int64).clamp(-int(pad), int(pad))
    ys = (torch.arange(H, device=x.device)[None, :] + s[:, 0:1]).clamp(0, H - 1)
    xs = (torch.arange(W, device=x.device)[None, :] + s[:, 1:2]).clamp(0, W - 1)
    rows = x.gather(2, ys[:, None, :, None].expand(B, C, H, W))
    return rows.gather(3, xs[:, None, None, :].expand(B, C, H, W))


def window(fn, iters):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0 = time.perf_counter()
    e0.record()
    for _ in range(iters):
        out = fn()
    e1.record()
    host = time.perf_counter() - t0
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters * 1e3, host / iters * 1e6, out


def alternate(fns, iters, warmup, rounds):
    for n, fn in fns.items():
        for _ in range(warmup[n]):
            fn()
    torch.cuda.synchronize()
    call, host = {n: [] for n in fns}, {n: [] for n in fns}
    for _ in range(rounds):
        for n, fn in fns.items():
            c, h, _ = window(fn, iters[n])
            call[n].append(c)
            host[n].append(h)
    med = lambda v: sorted(v)[len(v) // 2]      # noqa: E731
    return {n: {"call_us": round(med(call[n]), 1), "call_us_min_max": [round(min(call[n]), 1), round(max(call[n]), 1)], "host_us": round(med(host[n]), 1),
                "host_us_min_max": [round(min(host[n]), 1), round(max(host[n]), 1)], "window_calls": iters[n], "windows": rounds} for n in fns}


def traced(fn, iters=4):
    """Kernels and copies per call, from torch.profiler."""
    from torch.profiler import ProfilerActivity, profile
    fn()
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
        for _ in range(iters):
            fn()
        torch.cuda.synchronize()
    kernels = copies = 0
    for e in prof.events():
        if str(e.device_type).endswith("CUDA"):
            if e.name.lower().startswith(("memcpy", "memset")):
                copies += 1
            else:
                kernels += 1
    return {"launches": round(kernels / iters, 1), "copies": round(copies / iters, 1)}


def counted(fn):
    try:
        return traced(fn)
    except Exception as e:      # noqa: BLE001  (a profiler that does not start leaves the counts unmeasured, the timings stand)
        return {"launches": "not measured", "copies": "not measured", "profiler_error": repr(e)[:200]}


def host_rollout(image_dtype):
    """The host rollout after the reference's prepare(): (n_envs * T, ...) arrays, env-major.  Every page is written: one random slab of 64
    rows repeated (a never-touched array would be read from the kernel's zero page, which no real rollout is)."""
    g = np.random.default_rng(0)
    n = T * E
    img = np.empty((n, FS, H, W, 3), dtype=image_dtype)
    slab = g.integers(0, 256, (64, FS, H, W, 3), dtype=np.uint8) if image_dtype == np.uint8 else g.random((64, FS, H, W, 3), dtype=np.float32)
    img.reshape(n // 64, 64, FS, H, W, 3)[:] = slab
    tac = np.empty((n, FS, 3 * S, TH, TW), dtype=np.float32)
    tslab = (2 * g.random((64, FS, 3 * S, TH, TW), dtype=np.float32) - 1).astype(np.float32)
    tac.reshape(n // 64, 64, FS, 3 * S, TH, TW)[:] = tslab
    # make the rows distinct where it is cheap: the first element of every row carries the row number
    img[:, 0, 0, 0, 0] = (np.arange(n) % 251).astype(image_dtype)
    tac[:, 0, 0, 0, 0] = np.arange(n, dtype=np.float32) / n
    return {"image": img, "tactile": tac}


def device_store(host):
    """The store as the vec-env fills it, (T, n_envs, ...): row t * n_envs + env holds flat row env * T + t of the host rollout."""
    out = {}
    for k, v in host.items():
        d = torch.empty((T, E) + v.shape[1:], dtype=torch.from_numpy(v[:1]).dtype, device=DEV)
        for env in range(E):
            d[:, env].copy_(torch.from_numpy(v[env * T:(env + 1) * T]))
        out[k] = d
    torch.cuda.synchronize()
    return out


def run_variant(name, a):
    image_dtype = np.uint8 if name == "u8" else np.float32
    host = host_rollout(image_dtype)
    store = device_store(host)
    flat = {k: v.view((T * E,) + tuple(v.shape[2:])) for k, v in store.items()}
    n = T * E
    perm = np.random.default_rng(1).permutation(n).astype(np.int64)
    batches = [perm[i:i + B] for i in range(0, n, B)]
    d_idx = [torch.from_numpy(b).to(DEV) for b in batches]
    d_rows = [torch.from_numpy((b % T) * E + b // T).to(DEV) for b in batches]
    state = {"a": 0, "b": 0, "c": 0}

    def nxt(p):
        i = state[p]
        state[p] = (i + 1) % len(batches)
        return i

    def path_a():
        idx = batches[nxt("a")]
        obs = {k: torch.as_tensor(v[idx]).to(DEV) for k, v in host.items()}
        return vt_load(_flatten_frame_stack(obs), frame_stack=FS, device=DEV)

    def path_b():
        rows = d_rows[nxt("b")]
        obs = {k: v.index_select(0, rows) for k, v in flat.items()}
        return vt_load(_flatten_frame_stack(obs), frame_stack=FS, device=DEV)

    def path_c():
        return R.gather_load(store["image"], store["tactile"], d_idx[nxt("c")])

    # equal bits on one minibatch before anything is timed
    ra, rb, rc = path_a(), path_b(), path_c()
    torch.cuda.synchronize()
    for k in rc:
        assert torch.equal(ra[k], rc[k]) and torch.equal(rb[k], rc[k]), f"{name}: paths disagree on {k}"
    checksum = float(sum(v.double().sum() for v in rc.values()))

    fns = {"a_host": path_a, "b_resident": path_b, "c_gather_load": path_c}
    iters = {"a_host": a.host_iters, "b_resident": a.iters, "c_gather_load": a.iters}
    warm = {"a_host": 2, "b_resident": 20, "c_gather_load": 20}
    res = alternate(fns, iters, warm, a.rounds)
    for p, fn in fns.items():
        res[p].update(counted(fn))
    isz = 1 if name == "u8" else 4
    read = B * (FS * H * W * 3 * isz + FS * 3 * S * TH * TW * 4)
    write = B * (FS * H * W * 3 + FS * 3 * S * TH * TW) * 4
    c = res["c_gather_load"]
    c["bytes_read"], c["bytes_written"] = read, write
    for key, us in (("", c["call_us"]), ("_best", c["call_us_min_max"][0]), ("_worst", c["call_us_min_max"][1])):
        tbs = (read + write) / (us * 1e-6) / 1e12
        c["tbytes_per_s" + key] = round(tbs, 3)
        c["share_of_measured_copy_peak" + key] = round(tbs / HBM_COPY_TBS, 3)
        c["share_of_spec_peak" + key] = round(tbs / HBM_SPEC_TBS, 3)
    res["b_over_c"] = round(res["b_resident"]["call_us"] / c["call_us"], 2)
    res["a_over_c"] = round(res["a_host"]["call_us"] / c["call_us"], 1)
    res["store_gbytes"] = round(sum(v.numel() * v.element_size() for v in store.values()) / 1e9, 2)
    res["checksum"] = checksum
    return res


def device_frame_stores(image_dtype):
    """A frame store of random frames, ages and the stacked store the slot rule reads out of them, all made on the device."""
    g = torch.Generator(device=DEV).manual_seed(0)
    slots = T + FS - 1
    if image_dtype == np.uint8:
        img = torch.randint(0, 256, (slots, E, H, W, 3), dtype=torch.uint8, device=DEV, generator=g)
    else:
        img = torch.rand((slots, E, H, W, 3), dtype=torch.float32, device=DEV, generator=g)
    tac = torch.rand((slots, E, 3 * S, TH, TW), dtype=torch.float32, device=DEV, generator=g) * 2 - 1
    # ages as a rollout has them: episodes of 20 to 400 steps, so most stacks reach fs - 1 frames back and a few per cent are younger
    rng = np.random.default_rng(4)
    host_ages = np.empty((T, E), dtype=np.int32)
    for env in range(E):
        t = 0
        while t < T:
            n = int(rng.integers(20, 401))
            host_ages[t:t + n, env] = np.minimum(np.arange(min(n, T - t)), FS - 1)
            t += n
    ages = torch.from_numpy(host_ages).to(DEV)
    frames = {"image": img, "tactile": tac}
    stacked = {k: torch.empty((T, E, FS) + tuple(v.shape[2:]), dtype=v.dtype, device=DEV) for k, v in frames.items()}
    t, env = torch.arange(T, device=DEV)[:, None], torch.arange(E, device=DEV)[None, :]
    for k in range(FS):
        slot = t + (FS - 1) - torch.clamp(ages.long(), max=FS - 1 - k)
        for key in frames:
            stacked[key][:, :, k] = frames[key][slot, env]
    torch.cuda.synchronize()
    return frames, ages, stacked


def parent_gather(path):
    """m3l_rollout_gather_load of another build of the library (the parent commit's), called with `gather_load`'s arguments."""
    import ctypes as C
    from m3l_amd import _lib as L
    lib = C.CDLL(path)
    fn = lib.m3l_rollout_gather_load
    fn.restype, fn.argtypes = L._SIGS["m3l_rollout_gather_load"]

    def call(image_store, tactile_store, idx):
        B = idx.shape[0]
        img_out, tac_outs = R._loaded_outputs(B, FS, H, W, TH, TW, S, image_store.device)
        rc = fn(L.ptr(image_store), int(image_store.dtype == torch.uint8), H, W, 0.0, 1.0, L.ptr(img_out), L.ptr(tactile_store), 0, TH, TW, S, -1.0, 1.0,
                L.ptr_array(tac_outs), T, E, FS, L.ptr(idx), B, torch.cuda.current_stream().cuda_stream)
        assert rc == 0, "the parent library refused the call"
        return R._as_loaded(img_out, tac_outs)
    return call, int(lib.m3l_version())


def add_us(mode_kw, image_dtype, n=64):
    """Host time of one add() with a synchronise at the end of n of them, in microseconds; a buffer of n + 1 steps (the cost of an add() does not
    depend on the buffer's length)."""
    shapes = {"image": (FS, H, W, 3), "tactile": (FS, 3 * S, TH, TW)}
    buf = m3l_amd.DeviceRolloutBuffer(n + 1, E, shapes, {"image": image_dtype, "tactile": np.float32}, 4, device=DEV, **mode_kw)
    g = np.random.default_rng(2)
    obs = {"image": (g.integers(0, 256, (E,) + shapes["image"]).astype(image_dtype) if image_dtype == np.uint8 else
                     g.random((E,) + shapes["image"], dtype=np.float32)), "tactile": g.random((E,) + shapes["tactile"], dtype=np.float32)}
    act, z, start = np.zeros((E, 4), np.float32), np.zeros(E, np.float32), np.zeros(E, bool)
    buf.add(obs, act, z, np.ones(E, bool), z, z)      # allocates, and with frame_dedup uploads the whole stack
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(n):
        buf.add(obs, act, z, start, z, z)
    torch.cuda.synchronize()
    return round((time.perf_counter() - t0) / n * 1e6, 1)


def ppo_store_bytes(image_dtype):
    shapes = {"image": (FS, H, W, 3), "tactile": (FS, 3 * S, TH, TW)}
    mk = lambda **kw: m3l_amd.DeviceRolloutBuffer(T, E, shapes, {"image": image_dtype, "tactile": np.float32}, 4, device=DEV, **kw)      # noqa: E731
    return {"stacked": mk().store_bytes(), "frame_dedup": mk(frame_dedup=True).store_bytes()}


def run_aug_variant(name, a):
    image_dtype = np.uint8 if name == "u8" else np.float32
    pads = tuple(int(p) for p in a.pads.split(","))
    frames, ages, stacked = device_frame_stores(image_dtype)
    n = T * E
    perm = np.random.default_rng(1).permutation(n).astype(np.int64)
    d_idx = [torch.from_numpy(perm[i:i + B]).to(DEV) for i in range(0, n, B)]
    torch.manual_seed(3)
    d_shifts = [R._draw_shifts(pads, (B, 2, 2), torch.device(DEV)) for _ in d_idx]
    state = {}

    def nxt(p):
        i = state.get(p, 0)
        state[p] = (i + 1) % len(d_idx)
        return i

    def stacked_plain():
        return R.gather_load(stacked["image"], stacked["tactile"], d_idx[nxt("s")])

    def stacked_shift():
        i = nxt("ss")
        return R.gather_load(stacked["image"], stacked["tactile"], d_idx[i], shifts=d_shifts[i], shift_pad=pads)

    def frames_plain():
        return R.gather_load_frames(frames["image"], frames["tactile"], ages, d_idx[nxt("f")], FS)

    def frames_shift():
        i = nxt("fs")
        return R.gather_load_frames(frames["image"], frames["tactile"], ages, d_idx[i], FS, shifts=d_shifts[i], shift_pad=pads)

    def torch_shift():
        i = nxt("t")
        x = R.gather_load(stacked["image"], stacked["tactile"], d_idx[i])
        return {k: torch_shift_baseline(v, d_shifts[i][:, 0 if k == "image" else 1], pads[0 if k == "image" else 1]) for k, v in x.items()}

    fns = {"stacked": stacked_plain}
    if a.parent_lib:
        call, version = parent_gather(a.parent_lib)
        fns["stacked_parent"] = lambda: call(stacked["image"], stacked["tactile"], d_idx[nxt("p")])
        # the same launch of this build once more, in the window after the parent's: what the place in a round is worth
        fns["stacked_repeat"] = lambda: R.gather_load(stacked["image"], stacked["tactile"], d_idx[nxt("r")])
    if a.shift:
        fns["stacked_shift"] = stacked_shift
    if a.dedup:
        fns["frames"] = frames_plain
        if a.shift:
            fns["frames_shift"] = frames_shift
    if a.shift:
        fns["torch_shift"] = torch_shift
    # equal bits on one minibatch before anything is timed: every unshifted path against the stacked launch, every shifted path against the
    # torch ops on it
    first = {p: fn() for p, fn in fns.items()}
    torch.cuda.synchronize()
    for p, out in first.items():
        want = first["torch_shift"] if p.endswith("_shift") else first["stacked"]
        for k in want:
            assert torch.equal(out[k], want[k]), f"{name}: {p} disagrees on {k}"
    state.clear()
    res = alternate(fns, {p: a.iters for p in fns}, {p: 20 for p in fns}, a.rounds)
    for p, fn in fns.items():
        res[p].update(counted(fn))
    isz = 1 if name == "u8" else 4
    moved = B * (FS * H * W * 3 * isz + FS * 3 * S * TH * TW * 4) + B * (FS * H * W * 3 + FS * 3 * S * TH * TW) * 4
    for p in fns:
        if p != "torch_shift":
            tbs = moved / (res[p]["call_us"] * 1e-6) / 1e12
            res[p]["tbytes_per_s"], res[p]["share_of_measured_copy_peak"] = round(tbs, 3), round(tbs / HBM_COPY_TBS, 3)
    res["bytes_moved"] = moved
    if a.parent_lib:
        res["parent_lib_version"] = version
        lo, hi = res["stacked_parent"]["call_us_min_max"]
        res["parent_window_spread_us"] = round(hi - lo, 1)
        res["stacked_minus_parent_us"] = round(res["stacked"]["call_us"] - res["stacked_parent"]["call_us"], 1)
        res["stacked_repeat_minus_parent_us"] = round(res["stacked_repeat"]["call_us"] - res["stacked_parent"]["call_us"], 1)
    res["add_us"] = {"stacked": add_us({}, image_dtype), "frame_dedup": add_us({"frame_dedup": True}, image_dtype)}
    res["store_bytes"] = ppo_store_bytes(image_dtype)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5, help="alternating windows per path")
    ap.add_argument("--iters", type=int, default=200, help="calls per timed window of the device paths (b) and (c)")
    ap.add_argument("--host-iters", type=int, default=5, help="calls per timed window of the host path (a)")
    ap.add_argument("--variants", default="u8,f32")
    ap.add_argument("--shift", action="store_true", help="time the random-shift forms of the launch (see the docstring)")
    ap.add_argument("--dedup", action="store_true", help="time the launch on the frame-deduplicated store")
    ap.add_argument("--pads", default="4,2", help="image,tactile pads of --shift")
    ap.add_argument("--parent-lib", default=None, help="the parent commit's libm3l_amd.so, for the unshifted launch of both builds in one run")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("rollout_feed_bench: no GPU")
    out = {"shape": {"T": T, "n_envs": E, "frame_stack": FS, "image": [H, W, 3], "tactile": [3 * S, TH, TW], "B": B},
           "hbm_peak_tbytes_per_s": {"float4_copy_measured": HBM_COPY_TBS, "spec": HBM_SPEC_TBS}}
    for name in a.variants.split(","):
        out[name] = run_aug_variant(name, a) if a.shift or a.dedup else run_variant(name, a)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
