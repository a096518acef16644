"""Time of one SAC `replay_buffer.sample()` — from indices to (observations, next_observations, actions, dones, rewards) with both observation
dicts as the MAE's input tensors — at the reference's SAC shapes (EXPERIMENTS.md §5.21): a ring of T = 10000 steps of n_envs = 1 environment,
frame_stack = 4, image 64 x 64 x 3, 2 tactile sensors at 32 x 32 x 3; batches B = 64 and 256; two store variants, uint8 image + float32 tactile
and all float32; two store modes, a second store for the next observations and the single store (optimize_memory_usage).  Three paths:

  (a) host      what a user of the reference pays today (models/sac_mae.py:240, :253-260): numpy fancy index of both observation stores and the
                scalars on the host -> torch.as_tensor(...).to(device) from pageable memory -> _flatten_frame_stack -> vt_load, twice; the
                timeout mask and VecNormalize's reward normalisation in numpy
  (b) resident  the parent commit's means on device-resident stores: two calls of rollout.gather_load (with n_envs = 1 its swapped index is the
                row), index_select for the three scalars, torch ops for the mask and the normalisation.  The next rows of the single-store
                mode are computed outside the timed region
  (c) replay    m3l_amd.replay.gather_load + gather_rows: two launches

and, for the launch comparison alone, (b_obs) the two rollout.gather_load calls and (c_obs) the one replay.gather_load call.  Every call takes the
next B rows of one fixed permutation of the valid steps, so no path re-reads rows the caches still hold.  Before the timing the three paths'
outputs for one batch are compared bit for bit.

Timing, windows and launch counts are those of tools/rollout_feed_bench.py (device events around a window of back-to-back calls, the host clock
around the same window without its synchronise, paths alternated, median / min / max of --rounds windows; launches and copies from
torch.profiler in a run of their own).  For (c_obs): the bytes the algorithm needs — one read of 2 B stored rows, one write of 2 B float32
rows — over its call time, and the share of the 6.29 TB/s a float4 copy reaches on this chip.  Without a GPU the tool fails.

--dedup measures the frame-deduplicated store instead (EXPERIMENTS.md §5.23), at the same shapes, windows and alternation: (d_obs) one
replay.gather_load_frames call on frame stores against (c_obs) one replay.gather_load call on stacked stores holding the same data as rolling
stacks — compared bit for bit over every batch before the timing — with the bytes each needs (fs + 1 against 2 fs frame reads, equal writes),
`not_slower`: d_obs's median no higher than c_obs's median plus c_obs's own min-max spread; the host time of one add() in the four
layouts; and store_bytes() of 10^6 transitions at the reference's defaults.

--n-steps N measures n-step returns (EXPERIMENTS.md §5.24) on the stores of --dedup, full with pos = 0, with seeded scalars whose dones end
one walk in a hundred: the scalar launch, replay.nstep_rows(n_steps=N) against replay.gather_rows; the stacked gather fed rows and next_rows
against the one-list call (equal bytes); the frame-deduplicated gather fed both lists (2 fs frame reads a sample) against the one-list call
(fs + 1); and `sample()` of a DeviceReplayBuffer over the same stores with n_steps = 1 and N, stacked and frame-deduplicated.  The two-list
gathers are compared bit for bit with each other over every batch before the timing, and with n_steps = 1 against the one-list calls.
--parent-lib PATH adds, in the same alternation, the one-list gathers, gather_rows and `sample()` at n_steps = 1 through a second shared library
— one built from the parent commit — so that the default path of both commits is timed in one run: `*_parent` entries, their bits compared with
this commit's first, and `*_again` entries, this commit's own calls once more in a later slot of every round.  The spread of a path is the
largest of its two min-max ranges and of the gap between this commit's two slots (what the place in the alternation alone does to a median);
`default_path_within_spread`: every median of this commit no further from the parent's than that.

--per measures prioritised replay (EXPERIMENTS.md §5.25) on the stores of --dedup, full with pos = 0: `sample()` of a DeviceReplayBuffer with
prioritized=True against the uniform `sample()` of a buffer over the same stores, stacked and frame-deduplicated, and `update_priorities` of the
rows of a batch; the masses are seeded, log-uniform over six decades.  On bare priority arrays of --per-rows rows (10^6: the reference's
default buffer_size, no observation store needed): replay.per_sample against torch.cumsum + torch.searchsorted over all rows, and
replay.per_update against an index_put_ of (|td| + eps)^alpha, with the share of the torch pair's rows that have zero mass or differ from
per_sample's.  --parent-lib PATH adds the uniform `sample()`, gather_rows and the one-list gathers through the parent's library, as with
--n-steps.

Usage: python tools/replay_feed_bench.py [--rounds 5] [--iters 200] [--host-iters 5] [--variants u8,f32] [--batches 64,256]
                                         [--dedup | --n-steps N | --per] [--parent-lib PATH]
(one JSON line)"""
import argparse
import json
import math
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import m3l_amd  # noqa: E402,F401
from m3l_amd import replay as P  # noqa: E402
from m3l_amd import rollout as R  # noqa: E402
from m3l_amd import vt_load  # noqa: E402
from m3l_amd.fusion import _flatten_frame_stack  # noqa: E402
from rollout_feed_bench import HBM_COPY_TBS, HBM_SPEC_TBS, alternate, counted  # noqa: E402

DEV = "cuda:0"
T, E, FS, H, W, S, TH, TW, A = 10000, 1, 4, 64, 64, 2, 32, 32, 7
VAR, EPS, CLIP = 2.5, 1e-8, 10.0          # VecNormalize's running return variance (any positive value), epsilon and clip_reward defaults


def host_stores(image_dtype, seed):
    """(T, n_envs, ...) host stores with every page written: one random slab of 50 steps repeated, the first element of a step made distinct."""
    g = np.random.default_rng(seed)
    img = np.empty((T, E, FS, H, W, 3), dtype=image_dtype)
    slab = g.integers(0, 256, (50, E, FS, H, W, 3), dtype=np.uint8) if image_dtype == np.uint8 else g.random((50, E, FS, H, W, 3), dtype=np.float32)
    img.reshape(T // 50, 50, E, FS, H, W, 3)[:] = slab
    tac = np.empty((T, E, FS, 3 * S, TH, TW), dtype=np.float32)
    tac.reshape(T // 50, 50, E, FS, 3 * S, TH, TW)[:] = (2 * g.random((50, E, FS, 3 * S, TH, TW), dtype=np.float32) - 1).astype(np.float32)
    img[:, 0, 0, 0, 0, 0] = (np.arange(T) % 251).astype(image_dtype)
    tac[:, 0, 0, 0, 0, 0] = np.arange(T, dtype=np.float32) / T
    return {"image": img, "tactile": tac}


def run_config(name, single, B, host, host_next, store, store_next, scal, dscal, a):
    n_valid = T - 1 if single else T                  # a full single store with pos = 0: every step but step 0
    first = 1 if single else 0
    perm = (np.random.default_rng(1).permutation(n_valid) + first).astype(np.int64)
    batches = [perm[i:i + B] for i in range(0, n_valid - B + 1, B)]
    d_rows = [torch.from_numpy(b).to(DEV) for b in batches]
    d_next = [torch.from_numpy((b + 1) % T).to(DEV) for b in batches]
    scale = float(np.float32(math.sqrt(VAR + EPS)))
    d_scale = torch.tensor(scale, dtype=torch.float32, device=DEV)      # a device operand: torch turns a division by a host scalar into a multiplication
    state = {}

    def nxt(p):
        i = state.get(p, 0)
        state[p] = (i + 1) % len(batches)
        return i

    def load(obs):
        return vt_load(_flatten_frame_stack(obs), frame_stack=FS, device=DEV)

    def path_a():
        t = batches[nxt("a")]
        e = np.zeros_like(t)
        obs = load({k: torch.as_tensor(v[t, e]).to(DEV) for k, v in host.items()})
        src = host if single else host_next
        tn = (t + 1) % T if single else t
        nobs = load({k: torch.as_tensor(v[tn, e]).to(DEV) for k, v in src.items()})
        dones = scal["dones"][t, e] * (1 - scal["timeouts"][t, e])
        rewards = np.clip(scal["rewards"][t, e] / np.float32(scale), -CLIP, CLIP).astype(np.float32)
        up = lambda x: torch.as_tensor(x).to(DEV)      # noqa: E731
        return obs, nobs, up(scal["actions"][t, e]), up(dones.reshape(-1, 1)), up(rewards.reshape(-1, 1))

    def b_obs(i):
        obs = R.gather_load(store["image"], store["tactile"], d_rows[i])
        if single:
            return obs, R.gather_load(store["image"], store["tactile"], d_next[i])
        return obs, R.gather_load(store_next["image"], store_next["tactile"], d_rows[i])

    def path_b():
        i = nxt("b")
        obs, nobs = b_obs(i)
        rows = d_rows[i]
        actions = dscal["actions"].view(T * E, A).index_select(0, rows)
        dones = dscal["dones"].view(-1).index_select(0, rows) * (1 - dscal["timeouts"].view(-1).index_select(0, rows))
        rewards = torch.clamp(dscal["rewards"].view(-1).index_select(0, rows) / d_scale, -CLIP, CLIP)
        return obs, nobs, actions, dones.reshape(-1, 1), rewards.reshape(-1, 1)

    def c_obs(i):
        nx = store_next or {}
        return P.gather_load(store["image"], store["tactile"], d_rows[i], nx.get("image"), nx.get("tactile"))

    def path_c():
        i = nxt("c")
        obs, nobs = c_obs(i)
        actions, rewards, dones = P.gather_rows(dscal["actions"], dscal["rewards"], dscal["dones"], dscal["timeouts"], d_rows[i], scale, CLIP)
        return obs, nobs, actions, dones, rewards

    # equal bits on one batch before anything is timed
    ra, rb, rc = path_a(), path_b(), path_c()
    torch.cuda.synchronize()
    for x, y, z in zip(ra, rb, rc):
        for k in (z if isinstance(z, dict) else [None]):
            u, v, w = (q[k] if k is not None else q for q in (x, y, z))
            assert torch.equal(u, w) and torch.equal(v, w), f"{name}: paths disagree on {k or 'a scalar output'}"
    checksum = float(sum(v.double().sum() for d in rc[:2] for v in d.values()) + sum(t.double().sum() for t in rc[2:]))

    fns = {"a_host": path_a, "b_resident": path_b, "c_replay": path_c, "b_obs_two_launches": lambda: b_obs(nxt("bo")), "c_obs_one_launch": lambda: c_obs(nxt("co"))}
    iters = {n: (a.host_iters if n == "a_host" else a.iters) for n in fns}
    warm = {n: (2 if n == "a_host" else 20) for n in fns}
    res = alternate(fns, iters, warm, a.rounds)
    for p, fn in fns.items():
        res[p].update(counted(fn))
    isz = 1 if name == "u8" else 4
    read = 2 * B * (FS * H * W * 3 * isz + FS * 3 * S * TH * TW * 4)
    write = 2 * B * (FS * H * W * 3 + FS * 3 * S * TH * TW) * 4
    for p in ("b_obs_two_launches", "c_obs_one_launch"):
        c = res[p]
        c["bytes_read"], c["bytes_written"] = read, write
        for key, us in (("", c["call_us"]), ("_best", c["call_us_min_max"][0]), ("_worst", c["call_us_min_max"][1])):
            tbs = (read + write) / (us * 1e-6) / 1e12
            c["tbytes_per_s" + key] = round(tbs, 3)
            c["share_of_measured_copy_peak" + key] = round(tbs / HBM_COPY_TBS, 3)
    res["b_over_c"] = round(res["b_resident"]["call_us"] / res["c_replay"]["call_us"], 2)
    res["a_over_c"] = round(res["a_host"]["call_us"] / res["c_replay"]["call_us"], 1)
    res["b_obs_over_c_obs"] = round(res["b_obs_two_launches"]["call_us"] / res["c_obs_one_launch"]["call_us"], 3)
    res["checksum"] = checksum
    return res


def run_variant(name, a):
    image_dtype = np.uint8 if name == "u8" else np.float32
    host, host_next = host_stores(image_dtype, 0), host_stores(image_dtype, 5)
    store = {k: torch.from_numpy(v).to(DEV) for k, v in host.items()}
    store_next = {k: torch.from_numpy(v).to(DEV) for k, v in host_next.items()}
    g = np.random.default_rng(2)
    scal = dict(actions=g.standard_normal((T, E, A)).astype(np.float32), rewards=(3 * g.standard_normal((T, E))).astype(np.float32),
                dones=(g.random((T, E)) < 0.01).astype(np.float32))
    scal["timeouts"] = (scal["dones"] * (g.random((T, E)) < 0.5)).astype(np.float32)
    dscal = {k: torch.from_numpy(v).to(DEV) for k, v in scal.items()}
    torch.cuda.synchronize()
    out = {"store_gbytes_each": round(sum(v.numel() * v.element_size() for v in store.values()) / 1e9, 2)}
    for B in a.batches:
        out[f"B{B}_two_stores"] = run_config(name, False, B, host, host_next, store, store_next, scal, dscal, a)
        out[f"B{B}_single_store"] = run_config(name, True, B, host, None, store, None, scal, dscal, a)
    return out


# ---- the frame-deduplicated store (--dedup, EXPERIMENTS.md §5.23)
def dedup_stores(image_dtype, seed):
    """Device frame stores (T, n_envs, ...) of seeded frames, every one distinct in its first element, and the stacked stores that hold the same
    data as rolling stacks: one endless episode round the ring, so every step's stack is the fs frames up to its own (ages fs - 1 everywhere)
    and every step is valid in both layouts.  -> (frames, next_frames, stacked, stacked_next, stacked_single_next is the stacked store itself)."""
    g = np.random.default_rng(seed)

    def make(s):
        slab_i = g.integers(0, 256, (50, E, H, W, 3), dtype=np.uint8) if image_dtype == np.uint8 else g.random((50, E, H, W, 3), dtype=np.float32)
        img = np.tile(slab_i, (T // 50, 1, 1, 1, 1))
        tac = np.tile((2 * g.random((50, E, 3 * S, TH, TW), dtype=np.float32) - 1).astype(np.float32), (T // 50, 1, 1, 1, 1))
        img[:, 0, 0, 0, 0] = ((np.arange(T) + s) % 251).astype(image_dtype)
        tac[:, 0, 0, 0, 0] = (np.arange(T, dtype=np.float32) + s) / (2 * T)
        return {"image": torch.from_numpy(img).to(DEV), "tactile": torch.from_numpy(tac).to(DEV)}

    frames, next_frames = make(0), make(7)
    # obs[t, f] = frames[t - (fs - 1 - f)];  next_obs[t] = obs[t, 1:] + next_frames[t]
    stacked = {k: torch.stack([torch.roll(v, FS - 1 - f, 0) for f in range(FS)], dim=2).contiguous() for k, v in frames.items()}
    stacked_next = {k: torch.cat([stacked[k][:, :, 1:], next_frames[k].unsqueeze(2)], dim=2).contiguous() for k in frames}
    return frames, next_frames, stacked, stacked_next


def run_dedup_config(name, single, B, frames, next_frames, stacked, stacked_next, ages, a):
    perm = np.random.default_rng(1).permutation(T).astype(np.int64)
    d_rows = [torch.from_numpy(perm[i:i + B]).to(DEV) for i in range(0, T - B + 1, B)]
    state = {}

    def nxt(p):
        i = state.get(p, 0)
        state[p] = (i + 1) % len(d_rows)
        return i

    def c_stacked(i):
        nx = {} if single else stacked_next
        return P.gather_load(stacked["image"], stacked["tactile"], d_rows[i], nx.get("image"), nx.get("tactile"))

    def d_frames(i):
        nx = {} if single else next_frames
        return P.gather_load_frames(frames["image"], frames["tactile"], ages, d_rows[i], nx.get("image"), nx.get("tactile"), frame_stack=FS)

    # equal bits on every batch of the permutation before anything is timed
    for i in range(len(d_rows)):
        for x, y in zip(c_stacked(i), d_frames(i)):
            for k in x:
                assert torch.equal(x[k], y[k]), f"{name}: the stacked and the deduplicated store disagree on {k} (batch {i})"
    torch.cuda.synchronize()
    fns = {"c_obs_stacked": lambda: c_stacked(nxt("c")), "d_obs_frames": lambda: d_frames(nxt("d"))}
    res = alternate(fns, {n: a.iters for n in fns}, {n: 20 for n in fns}, a.rounds)
    for p, fn in fns.items():
        res[p].update(counted(fn))
    isz = 1 if name == "u8" else 4
    frame_in = H * W * 3 * isz + 3 * S * TH * TW * 4
    frame_out = (H * W * 3 + 3 * S * TH * TW) * 4
    for p, n_read in (("c_obs_stacked", 2 * FS), ("d_obs_frames", FS + 1)):
        c = res[p]
        c["bytes_read"], c["bytes_written"] = B * n_read * frame_in, B * 2 * FS * frame_out
        for key, us in (("", c["call_us"]), ("_best", c["call_us_min_max"][0]), ("_worst", c["call_us_min_max"][1])):
            tbs = (c["bytes_read"] + c["bytes_written"]) / (us * 1e-6) / 1e12
            c["tbytes_per_s" + key] = round(tbs, 3)
            c["share_of_measured_copy_peak" + key] = round(tbs / HBM_COPY_TBS, 3)
    s, d = res["c_obs_stacked"], res["d_obs_frames"]
    res["bytes_frames_over_stacked"] = round((d["bytes_read"] + d["bytes_written"]) / (s["bytes_read"] + s["bytes_written"]), 3)
    res["frames_over_stacked"] = round(d["call_us"] / s["call_us"], 3)
    spread = s["call_us_min_max"][1] - s["call_us_min_max"][0]
    res["stacked_spread_us"] = round(spread, 1)
    res["not_slower"] = bool(d["call_us"] <= s["call_us"] + spread)      # the condition for keeping the kernel's shape
    return res


def time_add(name, single, dedup, n_adds=400, T_add=2000):
    """Host time of one add() — the upload of one vec-env step from pageable numpy arrays — with a synchronise at the end of the window."""
    import time
    image_dtype = np.uint8 if name == "u8" else np.float32
    buf = m3l_amd.DeviceReplayBuffer(T_add, E, {"image": (FS, H, W, 3), "tactile": (FS, 3 * S, TH, TW)}, {"image": image_dtype, "tactile": np.float32}, A,
                                     optimize_memory_usage=single, handle_timeout_termination=not single, device=DEV, frame_dedup=dedup)
    g = np.random.default_rng(3)
    obs = {"image": (g.integers(0, 256, (E, FS, H, W, 3), dtype=np.uint8) if name == "u8" else g.random((E, FS, H, W, 3), dtype=np.float32)),
           "tactile": g.random((E, FS, 3 * S, TH, TW), dtype=np.float32)}
    rest = (np.zeros((E, A), np.float32), np.zeros(E, np.float32), np.zeros(E, bool), [{}] * E)
    times = []
    for r in range(6):                              # the first window allocates and warms up
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(n_adds):
            buf.add(obs, obs, *rest)
        torch.cuda.synchronize()
        times.append((time.perf_counter() - t0) / n_adds * 1e6)
    times = sorted(times[1:])
    return {"add_us": round(times[len(times) // 2], 1), "add_us_min_max": [round(times[0], 1), round(times[-1], 1)], "window_adds": n_adds}


def store_bytes_table():
    """store_bytes() of 10^6 transitions at the reference's defaults (arithmetic: nothing is allocated)."""
    shapes = {"image": (FS, H, W, 3), "tactile": (FS, 3 * S, TH, TW)}
    out = {}
    for dedup in (False, True):
        for single in (False, True):
            for img in ("u8", "f32"):
                b = m3l_amd.DeviceReplayBuffer(1_000_000, 1, shapes, {"image": np.uint8 if img == "u8" else np.float32, "tactile": np.float32}, A,
                                               optimize_memory_usage=single, handle_timeout_termination=not single, device=DEV, frame_dedup=dedup)
                out[f"{'frames' if dedup else 'stacked'}_{'single_store' if single else 'two_stores'}_{img}"] = b.store_bytes()["total"]
    return out


def run_dedup(a):
    out = {"store_bytes_1e6_transitions": store_bytes_table()}
    ages = torch.full((T, E), FS - 1, dtype=torch.int32, device=DEV)
    for name in a.variants.split(","):
        frames, next_frames, stacked, stacked_next = dedup_stores(np.uint8 if name == "u8" else np.float32, 0)
        torch.cuda.synchronize()
        out[name] = {}
        for B in a.batches:
            out[name][f"B{B}_two_stores"] = run_dedup_config(name, False, B, frames, next_frames, stacked, stacked_next, ages, a)
            out[name][f"B{B}_single_store"] = run_dedup_config(name, True, B, frames, None, stacked, None, ages, a)
        del frames, next_frames, stacked, stacked_next
        torch.cuda.empty_cache()
        out[name]["add"] = {f"{'frames' if dedup else 'stacked'}_{'single_store' if single else 'two_stores'}": time_add(name, single, dedup)
                            for dedup in (False, True) for single in (False, True)}
    return out


# ---- n-step returns (--n-steps, EXPERIMENTS.md §5.24)
def through_library(path):
    """-> wrap(fn): fn with every m3l_amd call going through the shared library at `path` (the bindings of m3l_amd._lib that it exports)."""
    import ctypes as C
    from m3l_amd import _lib as L
    other = C.CDLL(path)
    for sym, (res, args) in L._SIGS.items():
        if hasattr(other, sym):
            getattr(other, sym).restype, getattr(other, sym).argtypes = res, args
    own = L.lib()

    def wrap(fn):
        def call():
            L._lib = other
            try:
                return fn()
            finally:
                L._lib = own
        return call
    return wrap


def seeded_mass(n, seed):
    """n masses, log-uniform over [1e-3, 1e3], on the device."""
    g = np.random.default_rng(seed)
    return torch.from_numpy(np.exp(g.uniform(np.log(1e-3), np.log(1e3), n)).astype(np.float32)).to(DEV)


def resident_buffer(image_dtype, frame_dedup, n_steps, stores, next_stores, ages, dscal, prioritized=False):
    """A full DeviceReplayBuffer (pos = 0) standing on stores that are already on the device.  prioritized: with seeded masses on its valid
    steps (the frame-deduplicated ring does not sample its fs - 1 oldest)."""
    shapes = {"image": (FS, H, W, 3), "tactile": (FS, 3 * S, TH, TW)}
    buf = m3l_amd.DeviceReplayBuffer(T * E, E, shapes, {"image": image_dtype, "tactile": np.float32}, A, device=DEV, frame_dedup=frame_dedup,
                                     n_steps=n_steps, gamma=0.99, prioritized=prioritized)
    if prioritized:
        buf.mass = seeded_mass(T * E, 4).reshape(T, E)
        if frame_dedup:
            buf.mass[:FS - 1] = 0
        buf.block_mass, buf.block_min = P.per_refresh(buf.mass)
        buf.max_priority = torch.ones(1, dtype=torch.float32, device=DEV)
    if frame_dedup:
        buf.frames, buf.next_frames, buf.ages = stores, next_stores, ages
    else:
        buf.observations, buf.next_observations = stores, next_stores
    buf.actions, buf.rewards, buf.dones, buf.timeouts = (dscal[k] for k in ("actions", "rewards", "dones", "timeouts"))
    buf.pos, buf.full = 0, True
    return buf


def run_nstep_config(name, B, n, frames, next_frames, stacked, stacked_next, ages, dscal, a):
    image_dtype = np.uint8 if name == "u8" else np.float32
    perm = np.random.default_rng(1).permutation(T).astype(np.int64)
    d_rows = [torch.from_numpy(perm[i:i + B]).to(DEV) for i in range(0, T - B + 1, B)]
    scale, newest = float(np.float32(math.sqrt(VAR + EPS))), T - 1
    sc = (dscal["actions"], dscal["rewards"], dscal["dones"], dscal["timeouts"])
    walks = [P.nstep_rows(*sc, r, n, 0.99, newest, scale, CLIP) for r in d_rows]
    d_next = [w[5] for w in walks]
    moved = float(np.mean([(w[5] != w[4]).double().mean().item() for w in walks]))
    state = {}

    def nxt(p):
        i = state.get(p, 0)
        state[p] = (i + 1) % len(d_rows)
        return i

    def stacked_call(i, two):
        return P.gather_load(stacked["image"], stacked["tactile"], d_rows[i], stacked_next["image"], stacked_next["tactile"],
                             next_rows=d_next[i] if two else None)

    def frames_call(i, two):
        return P.gather_load_frames(frames["image"], frames["tactile"], ages, d_rows[i], next_frames["image"], next_frames["tactile"],
                                    next_rows=d_next[i] if two else None, frame_stack=FS)

    def same(x, y, what):
        for u, v in zip(x, y):
            for k in u:
                assert torch.equal(u[k], v[k]), f"{name} B={B}: {what} disagree on {k}"
    for i in range(len(d_rows)):
        same(stacked_call(i, True), frames_call(i, True), "the stacked and the deduplicated two-list gathers")
    one = P.nstep_rows(*sc, d_rows[0], 1, 0.99, newest, scale, CLIP)
    ref = P.gather_rows(*sc, d_rows[0], scale, CLIP, return_rows=True)
    assert all(torch.equal(x, y) for x, y in zip(ref, (one[0], one[1], one[2], one[4]))) and torch.equal(one[5], one[4])
    saved = d_next[0]
    d_next[0] = one[5]
    same(stacked_call(0, True), stacked_call(0, False), "the two-list stacked gather with next_rows = rows and the one-list call")
    same(frames_call(0, True), frames_call(0, False), "the two-list deduplicated gather with next_rows = rows and the one-list call")
    d_next[0] = saved
    bufs = {(dedup, k): resident_buffer(image_dtype, dedup, k, frames if dedup else stacked, next_frames if dedup else stacked_next, ages, dscal)
            for dedup in (False, True) for k in (1, n)}
    env = type("Env", (), dict(norm_obs=False, norm_reward=True, ret_rms=type("Rms", (), dict(var=VAR)), epsilon=EPS, clip_reward=CLIP))
    torch.cuda.synchronize()
    fns = {"rows_gather_rows": lambda: P.gather_rows(*sc, d_rows[nxt("r1")], scale, CLIP, return_rows=True),
           "rows_nstep_rows": lambda: P.nstep_rows(*sc, d_rows[nxt("rn")], n, 0.99, newest, scale, CLIP),
           "stacked_one_list": lambda: stacked_call(nxt("s1"), False), "stacked_two_lists": lambda: stacked_call(nxt("s2"), True),
           "frames_one_list": lambda: frames_call(nxt("f1"), False), "frames_two_lists": lambda: frames_call(nxt("f2"), True)}
    for (dedup, k), buf in bufs.items():
        fns[f"sample_{'frames' if dedup else 'stacked'}_n{k}"] = (lambda b: lambda: b.sample(B, env=env))(buf)
    default_path = ("rows_gather_rows", "stacked_one_list", "frames_one_list", "sample_stacked_n1", "sample_frames_n1")
    if a.parent_lib:
        wrap = through_library(a.parent_lib)
        for p in default_path:
            fns[p + "_parent"] = wrap(fns[p])
        for p in default_path:
            fns[p + "_again"] = (lambda f: lambda: f())(fns[p])
        state.clear()
        for p in default_path[:3]:                    # the same batch through both libraries: equal bits
            state.clear()
            mine = fns[p]()
            state.clear()
            theirs = fns[p + "_parent"]()
            for x, y in zip(mine, theirs):
                for k in (x if isinstance(x, dict) else [None]):
                    assert torch.equal(x[k] if k is not None else x, y[k] if k is not None else y), f"{name} B={B}: {p} differs from the parent library"
    res = alternate(fns, {p: a.iters for p in fns}, {p: 20 for p in fns}, a.rounds)
    for p, fn in fns.items():
        res[p].update(counted(fn))
    if a.parent_lib:
        res["default_path_vs_parent"] = {}
        for p in default_path:
            mine, theirs, again = res[p], res[p + "_parent"], res[p + "_again"]
            spread = max(theirs["call_us_min_max"][1] - theirs["call_us_min_max"][0], mine["call_us_min_max"][1] - mine["call_us_min_max"][0],
                         abs(mine["call_us"] - again["call_us"]))
            res["default_path_vs_parent"][p] = {"this_us": mine["call_us"], "parent_us": theirs["call_us"], "this_again_us": again["call_us"],
                                                "spread_us": round(spread, 1), "within_spread": bool(abs(mine["call_us"] - theirs["call_us"]) <= spread)}
        res["default_path_within_spread"] = all(v["within_spread"] for v in res["default_path_vs_parent"].values())
    isz = 1 if name == "u8" else 4
    frame_in = H * W * 3 * isz + 3 * S * TH * TW * 4
    frame_out = (H * W * 3 + 3 * S * TH * TW) * 4
    for p, n_read in (("stacked_one_list", 2 * FS), ("stacked_two_lists", 2 * FS), ("frames_one_list", FS + 1), ("frames_two_lists", 2 * FS)):
        c = res[p]
        c["bytes_read"], c["bytes_written"] = B * n_read * frame_in, B * 2 * FS * frame_out
        for key, us in (("", c["call_us"]), ("_best", c["call_us_min_max"][0]), ("_worst", c["call_us_min_max"][1])):
            tbs = (c["bytes_read"] + c["bytes_written"]) / (us * 1e-6) / 1e12
            c["tbytes_per_s" + key] = round(tbs, 3)
            c["share_of_measured_copy_peak" + key] = round(tbs / HBM_COPY_TBS, 3)
    for num, den in (("rows_nstep_rows", "rows_gather_rows"), ("stacked_two_lists", "stacked_one_list"), ("frames_two_lists", "frames_one_list"),
                     (f"sample_stacked_n{n}", "sample_stacked_n1"), (f"sample_frames_n{n}", "sample_frames_n1")):
        res[f"{num}_over_{den}"] = round(res[num]["call_us"] / res[den]["call_us"], 3)
    res["share_of_walks_that_move"] = round(moved, 4)
    return res


def run_nstep(a):
    n = a.n_steps
    ages = torch.full((T, E), FS - 1, dtype=torch.int32, device=DEV)
    g = np.random.default_rng(2)
    scal = dict(actions=g.standard_normal((T, E, A)).astype(np.float32), rewards=(3 * g.standard_normal((T, E))).astype(np.float32),
                dones=(g.random((T, E)) < 0.01).astype(np.float32))
    scal["timeouts"] = (scal["dones"] * (g.random((T, E)) < 0.5)).astype(np.float32)
    dscal = {k: torch.from_numpy(v).to(DEV) for k, v in scal.items()}
    out = {"n_steps": n}
    for name in a.variants.split(","):
        frames, next_frames, stacked, stacked_next = dedup_stores(np.uint8 if name == "u8" else np.float32, 0)
        torch.cuda.synchronize()
        out[name] = {f"B{B}": run_nstep_config(name, B, n, frames, next_frames, stacked, stacked_next, ages, dscal, a) for B in a.batches}
        del frames, next_frames, stacked, stacked_next
        torch.cuda.empty_cache()
    return out


# ---- prioritised replay (--per, EXPERIMENTS.md §5.25)
def parent_entries(fns, default_path, parent_lib):
    """The default path through the parent's library and once more through this one, as run_nstep_config does it."""
    wrap = through_library(parent_lib)
    for p in default_path:
        fns[p + "_parent"] = wrap(fns[p])
    for p in default_path:
        fns[p + "_again"] = (lambda f: lambda: f())(fns[p])


def parent_verdict(res, default_path):
    res["default_path_vs_parent"] = {}
    for p in default_path:
        mine, theirs, again = res[p], res[p + "_parent"], res[p + "_again"]
        spread = max(theirs["call_us_min_max"][1] - theirs["call_us_min_max"][0], mine["call_us_min_max"][1] - mine["call_us_min_max"][0],
                     abs(mine["call_us"] - again["call_us"]))
        res["default_path_vs_parent"][p] = {"this_us": mine["call_us"], "parent_us": theirs["call_us"], "this_again_us": again["call_us"],
                                            "spread_us": round(spread, 1), "within_spread": bool(abs(mine["call_us"] - theirs["call_us"]) <= spread)}
    res["default_path_within_spread"] = all(v["within_spread"] for v in res["default_path_vs_parent"].values())


def run_per_config(name, B, frames, next_frames, stacked, stacked_next, ages, dscal, a):
    image_dtype = np.uint8 if name == "u8" else np.float32
    perm = np.random.default_rng(1).permutation(T).astype(np.int64)
    d_rows = [torch.from_numpy(perm[i:i + B]).to(DEV) for i in range(0, T - B + 1, B)]
    scale = float(np.float32(math.sqrt(VAR + EPS)))
    sc = (dscal["actions"], dscal["rewards"], dscal["dones"], dscal["timeouts"])
    env = type("Env", (), dict(norm_obs=False, norm_reward=True, ret_rms=type("Rms", (), dict(var=VAR)), epsilon=EPS, clip_reward=CLIP))
    bufs = {(dedup, per): resident_buffer(image_dtype, dedup, 1, frames if dedup else stacked, next_frames if dedup else stacked_next, ages, dscal, per)
            for dedup in (False, True) for per in (False, True)}
    # a prioritised batch is the uniform buffer's batch of the same rows, and every row has positive mass
    for dedup in (False, True):
        batch = bufs[dedup, True].sample(B, env=env)
        rows = batch.rows.cpu()
        assert bool((bufs[dedup, True].mass.reshape(-1)[batch.rows] > 0).all())
        base = bufs[dedup, False].sample(1, env=env, indices=(rows // E, rows % E))
        for fld in base._fields:
            x, y = getattr(batch, fld), getattr(base, fld)
            for k in (x if isinstance(x, dict) else [None]):
                assert torch.equal(x[k] if k is not None else x, y[k] if k is not None else y), f"{name} B={B}: {fld} differs from the uniform buffer"
    g = torch.Generator(device=DEV).manual_seed(3)
    tds = [torch.randn(B, 1, generator=g, device=DEV) for _ in range(8)]
    upd_rows = [bufs[False, True].sample(B).rows for _ in range(8)]
    state = {}

    def nxt(p, n):
        i = state.get(p, 0)
        state[p] = (i + 1) % n
        return i

    def update():
        i = nxt("u", 8)
        bufs[False, True].update_priorities(upd_rows[i], tds[i])
    torch.cuda.synchronize()
    fns = {"update_priorities": update}
    for (dedup, per), buf in bufs.items():
        fns[f"sample_{'frames' if dedup else 'stacked'}_{'per' if per else 'uniform'}"] = (lambda b: lambda: b.sample(B, env=env))(buf)
    default_path = ("rows_gather_rows", "stacked_one_list", "frames_one_list", "sample_stacked_uniform", "sample_frames_uniform")
    if a.parent_lib:
        fns["rows_gather_rows"] = lambda: P.gather_rows(*sc, d_rows[nxt("r1", len(d_rows))], scale, CLIP, return_rows=True)
        fns["stacked_one_list"] = lambda: P.gather_load(stacked["image"], stacked["tactile"], d_rows[nxt("s1", len(d_rows))], stacked_next["image"],
                                                        stacked_next["tactile"])
        fns["frames_one_list"] = lambda: P.gather_load_frames(frames["image"], frames["tactile"], ages, d_rows[nxt("f1", len(d_rows))],
                                                              next_frames["image"], next_frames["tactile"], frame_stack=FS)
        parent_entries(fns, default_path, a.parent_lib)
        for p in default_path[:3]:                    # the same batch through both libraries: equal bits
            state.clear()
            mine = fns[p]()
            state.clear()
            theirs = fns[p + "_parent"]()
            for x, y in zip(mine, theirs):
                for k in (x if isinstance(x, dict) else [None]):
                    assert torch.equal(x[k] if k is not None else x, y[k] if k is not None else y), f"{name} B={B}: {p} differs from the parent library"
    res = alternate(fns, {p: a.iters for p in fns}, {p: 20 for p in fns}, a.rounds)
    for p, fn in fns.items():
        res[p].update(counted(fn))
    if a.parent_lib:
        parent_verdict(res, default_path)
    for lay in ("stacked", "frames"):
        res[f"sample_{lay}_per_over_uniform"] = round(res[f"sample_{lay}_per"]["call_us"] / res[f"sample_{lay}_uniform"]["call_us"], 3)
    return res


def run_per_bare(B, a):
    """The priority structure alone at --per-rows rows against the torch ops a user would write on the same device."""
    n, alpha, eps = a.per_rows, 0.6, 1e-6
    mass = seeded_mass(n, 6)
    mass[torch.rand(n, device=DEV) < 0.2] = 0           # steps outside the valid window, dead rows: a fifth zero
    bm, bmin = P.per_refresh(mass)
    mp = torch.ones(1, dtype=torch.float32, device=DEV)
    torch_mass = mass.clone()
    g = torch.Generator(device=DEV).manual_seed(7)
    us = [torch.rand(B, generator=g, device=DEV) for _ in range(16)]
    tds = [torch.randn(B, generator=g, device=DEV) for _ in range(16)]
    rows = [P.per_sample(mass, bm, bmin, u)[0] for u in us]
    ar = torch.arange(B, dtype=torch.float32, device=DEV)
    state = {}

    def nxt(p):
        i = state.get(p, 0)
        state[p] = (i + 1) % 16
        return i

    def torch_sample(i=None):
        u = us[nxt("ts") if i is None else i]
        c = torch.cumsum(torch_mass, 0)
        return torch.searchsorted(c, (ar + u) * (c[-1] / B), right=True)

    def torch_update():
        i = nxt("tu")
        torch_mass.index_put_((rows[i],), (tds[i].abs() + eps).pow(alpha))

    def per_update():
        i = nxt("pu")
        P.per_update(mass, bm, bmin, mp, rows[i], tds[i], alpha, eps)
    # before anything is updated both hold the same masses: how the torch pair's rows compare
    zero = differ = 0
    for i in range(16):
        r = torch_sample(i).clamp(max=n - 1)
        zero += int((mass[r] == 0).sum())
        differ += int((r != rows[i]).sum())
    torch.cuda.synchronize()
    fns = {"per_sample": lambda: P.per_sample(mass, bm, bmin, us[nxt("ps")]), "torch_cumsum_searchsorted": torch_sample, "per_update": per_update,
           "torch_index_put": torch_update}
    res = alternate(fns, {p: a.iters for p in fns}, {p: 20 for p in fns}, a.rounds)
    for p, fn in fns.items():
        res[p].update(counted(fn))
    res["rows"] = n
    res["torch_rows_of_zero_mass"] = [zero, 16 * B]
    res["torch_rows_that_differ_from_per_sample"] = [differ, 16 * B]
    res["per_sample_over_torch"] = round(res["per_sample"]["call_us"] / res["torch_cumsum_searchsorted"]["call_us"], 3)
    res["per_update_over_torch"] = round(res["per_update"]["call_us"] / res["torch_index_put"]["call_us"], 3)
    return res


def run_per(a):
    ages = torch.full((T, E), FS - 1, dtype=torch.int32, device=DEV)
    g = np.random.default_rng(2)
    scal = dict(actions=g.standard_normal((T, E, A)).astype(np.float32), rewards=(3 * g.standard_normal((T, E))).astype(np.float32),
                dones=(g.random((T, E)) < 0.01).astype(np.float32))
    scal["timeouts"] = (scal["dones"] * (g.random((T, E)) < 0.5)).astype(np.float32)
    dscal = {k: torch.from_numpy(v).to(DEV) for k, v in scal.items()}
    out = {"bare": {f"B{B}": run_per_bare(B, a) for B in a.batches}}
    for name in a.variants.split(","):
        frames, next_frames, stacked, stacked_next = dedup_stores(np.uint8 if name == "u8" else np.float32, 0)
        torch.cuda.synchronize()
        out[name] = {f"B{B}": run_per_config(name, B, frames, next_frames, stacked, stacked_next, ages, dscal, a) for B in a.batches}
        del frames, next_frames, stacked, stacked_next
        torch.cuda.empty_cache()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5, help="alternating windows per path")
    ap.add_argument("--iters", type=int, default=200, help="calls per timed window of the device paths")
    ap.add_argument("--host-iters", type=int, default=5, help="calls per timed window of the host path (a)")
    ap.add_argument("--variants", default="u8,f32")
    ap.add_argument("--batches", default="64,256")
    ap.add_argument("--dedup", action="store_true", help="measure the frame-deduplicated store against the stacked one instead of the three paths")
    ap.add_argument("--n-steps", type=int, default=0, help="measure n-step returns with this n_steps (>= 2) instead of the three paths")
    ap.add_argument("--per", action="store_true", help="measure prioritised replay instead of the three paths")
    ap.add_argument("--per-rows", type=int, default=1_000_000, help="with --per: rows of the bare priority arrays")
    ap.add_argument("--parent-lib", default=None, help="with --n-steps or --per: a shared library built from the parent commit, timed on the default path")
    a = ap.parse_args()
    if a.n_steps and (a.n_steps < 2 or a.dedup):
        raise SystemExit("replay_feed_bench: --n-steps takes a value of at least 2 and excludes --dedup")
    if a.per and (a.n_steps or a.dedup):
        raise SystemExit("replay_feed_bench: --per excludes --dedup and --n-steps")
    a.batches = [int(b) for b in a.batches.split(",")]
    if not torch.cuda.is_available():
        raise SystemExit("replay_feed_bench: no GPU")
    out = {"shape": {"T": T, "n_envs": E, "frame_stack": FS, "image": [H, W, 3], "tactile": [3 * S, TH, TW], "B": a.batches, "action_dim": A},
           "hbm_peak_tbytes_per_s": {"float4_copy_measured": HBM_COPY_TBS, "spec": HBM_SPEC_TBS}}
    if a.dedup or a.n_steps or a.per:
        out.update({"prioritized": run_per(a)} if a.per else {"n_step": run_nstep(a)} if a.n_steps else {"frame_dedup": run_dedup(a)})
        print(json.dumps(out))
        return
    for name in a.variants.split(","):
        out[name] = run_variant(name, a)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
