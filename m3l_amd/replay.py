"""The SAC replay buffer kept on the GPU: `DeviceReplayBuffer` stands where `SAC_MAE` uses SB3's `DictReplayBuffer`, and a batch leaves it with
both observation dicts as the MAE's input tensors (csrc/replay.hip, include/m3l_amd.h "device-resident replay buffer").

Reference path replaced, per gradient step (models/sac_mae.py): `self.replay_buffer.sample(batch_size, env=self._vec_normalize_env)` (:240) —
SB3 fancy-indexes `observations` and `next_observations` on the host and uploads both from pageable memory — the frame-stack permute of both
(:253-260), `vt_load` of both, and the repeated load of the same rows inside the features extractor at every actor / critic call.  Here

    replay_data = buffer.sample(batch_size, env=vec_normalize_env)
    mae_loss = mae(replay_data.observations)                     # a LoadedObs: the extractors take it as it is
    features = extractor(replay_data.observations)               # one load feeds the MAE, the actor and both critic calls
    target_q = head.td_target(extractor(replay_data.next_observations), replay_data.rewards, replay_data.dones, gamma, ...)

The stores keep the layout the vec-env fills them in, (T, n_envs, ...), and a row number is t * n_envs + e.  `sample(indices=...)` is the parity
seam (what `get(indices=...)` is for the rollout).  A sample is three launches: the index draw, the observations, the scalars.

SB3 is not in the reference tree: the ring (`add`, `pos`, `full`), the single-store mode (`optimize_memory_usage`), the timeout mask and
`VecNormalize.normalize_reward` are restated here and in tests/replay_cases.py (parity unpinned).  Not covered: `save_replay_buffer` pickling,
HER, observation normalisation (`norm_obs`).

`n_steps=n > 1` gives n-step returns (SB3's `NStepReplayBuffer` / `SAC(n_steps=)` from 2.7, restated in tests/nstep_cases.py, parity unpinned).
From a sampled (t, e) the walk goes towards newer steps and ends at `last = (t + k*) % T`, k* the smallest k in [0, n - 1] at which
`dones[(t + k) % T, e] != 0` (a truncated step is stored with done = 1 too) or `(t + k) % T` is the step written last, else n - 1: it crosses
neither an episode end nor the write head.  With g = float32(gamma): rewards = sum_{k <= k*} g^k r[(t + k) % T, e] of the (normalised)
rewards, g^k by repeated float32 multiplication and the sum in float32 in ascending k; dones = dones[last] * (1 - timeouts[last]);
discounts = g^(k* + 1); observations, actions and rows are those of (t, e); next_observations is the next observation of (last, e) and
next_rows = last * n_envs + e.  `sample()` returns an `NStepReplayBatch` and stays three launches with nothing read back: the draw,
`nstep_rows` (m3l_replay_nstep_rows) and one observation gather fed `rows` and `next_rows` (m3l_replay_gather_load_rows2 /
m3l_replay_gather_load_frames_rows2).  `head.td_target(extractor(batch.next_observations), batch.rewards, batch.dones, batch.discounts, ...)`
takes the per-row discount.  The single-store mode is refused, as SB3 refuses it: it has no agreed next observation at `last`.

`frame_dedup=True` stores every frame once.  The reference's `FrameStack` wrapper (utils/frame_stack.py:76-105) makes each observation the last
`fs` frames of its episode, so the stacked stores hold one frame `fs` times each; the deduplicated stores `frames` / `next_frames` hold the
newest frame of each observation, `ages` says how far back a step's stack reaches into its episode, and `gather_load_frames` puts both stacks of
a sample together from fs + 1 frames (m3l_replay_gather_load_frames).  At the reference's shapes 10^6 transitions take 73.8 GB instead of
295 GB.  The wrapper and the vec-env's auto-reset are restated in tests/replay_frame_cases.py (parity unpinned).

`prioritized=True` gives proportional prioritised replay (Schaul et al. 2016; neither the reference tree nor SB3 has it: restated in float64 in
tests/per_cases.py, parity unpinned) without a host-side sum tree and without reading a TD error back.  `mass` (T, n_envs) holds
priority^alpha per row, priority = |td| + priority_eps, and 0 for every row outside `_valid_steps()`; `block_mass` / `block_min` hold the sum
and the smallest positive leaf of each run of PER_BLOCK rows, always recomputed from the leaves (no drift, no float atomics); `max_priority`
starts at 1 and never decreases.  add() gives the new step max_priority^alpha and zeroes the steps that left the valid window (two launches).
`sample()`: total = sum(block_mass); x_k = (k + u_k) * (total / B) (stratified, as in the paper); the block is the first whose inclusive
prefix exceeds x_k, the row the first leaf of it whose inclusive prefix exceeds the rest of x_k, where rounding leaves none the last of positive
mass: a row of zero mass is never returned.  weights = (min mass / mass[row])^beta.  `update_priorities(rows, td)`: a non-finite td takes the
max_priority of before the call, a row of zero mass or outside the ring is skipped, of duplicate rows the largest priority wins.  The loop:

    batch = buffer.sample(batch_size, env=vec_normalize_env, beta=beta_t)                       # a PrioritizedReplayBatch
    target_q = head.td_target(extractor(batch.next_observations), batch.rewards, batch.dones, batch.discounts, ...)
    critic_loss, td = head.critic_loss(features, batch.actions, target_q, weights=batch.weights, return_td_errors=True)
    buffer.update_priorities(batch.rows, td)

`random_shift=p` (or `dict(image=p_i, tactile=p_t)`) gives the random-shift augmentation of DrQ (Kostrikov et al. 2021) and RAD (Laskin et al.
2020): replicate-pad a frame by p pixels and crop it at a random offset.  Neither the reference tree nor SB3 has it: restated in
tests/shift_cases.py, parity unpinned.  `shifts` (B, 2, 2, 2) int32 holds one (dy, dx) per [sample, half (0 observations, 1 next
observations), modality (0 image, 1 tactile)]: all frames of the stack, all three channels and all sensors share it, the two halves are drawn
independently, and the kernel clamps every entry to [-p, p].  With x the unaugmented LoadedObs tensor of a half, (B, 3 fs, H, W),

    out[b, c, y, x] = x[b, c, clamp(y + dy, 0, H - 1), clamp(x + dx, 0, W - 1)]

which is `F.pad(x, (p, p, p, p), mode="replicate")[..., p + dy : p + dy + H, p + dx : p + dx + W]`, and the normalisation is elementwise, so an
augmented batch has the bits of that indexing applied to the unaugmented batch of the same rows.  The shift is an address change on the read
side of the same one gather launch (m3l_replay_gather_load_shift / m3l_replay_gather_load_frames_shift); `sample()` draws the shifts with one
torch.randint per distinct nonzero pad on the device, reads nothing back and keeps them in `last_shifts`.  Both LoadedObs are augmented, so
`mae(x)`, the actor and the critics all see the shifted observations; `sample(indices=..., shifts=torch.zeros(...))` gives the unaugmented
batch of the same rows.  DrQ's averaging over K and M augmentations is the caller's loop over `sample(indices=...)`.
"""
import math
from typing import NamedTuple

import numpy as np
import torch

from . import _lib as L
from .functional import _require_cuda
from .pretrain_utils import LoadedObs
from .rollout import (MAX_SHIFT_PAD, _as_loaded, _check_obs, _check_pad, _check_shift_pad, _check_shifts, _check_stores,  # noqa: F401
                      _draw_shifts, _loaded_outputs, _obs_spec, _require_device, _shift_pads, _stream)


def _check_rows(who, rows):
    _require_cuda(rows, who + ": rows")
    if rows.dtype != torch.int64 or rows.dim() != 1 or not rows.is_contiguous():
        raise ValueError(f"{who}: rows must be a contiguous 1-D int64 tensor")


def _check_next_rows(who, next_rows, rows):
    _require_cuda(next_rows, who + ": next_rows")
    if next_rows.dtype != torch.int64 or next_rows.shape != rows.shape or not next_rows.is_contiguous():
        raise ValueError(f"{who}: next_rows must be a contiguous int64 tensor of rows' shape {tuple(rows.shape)}")


def _gather_load(who, kind, image, tactile, rows, image_next, tactile_next, image_normalization, tactile_normalization, row_shift, next_rows,
                 ages=None, frame_stack=None, shifts=None, shift_pad=(0, 0)):
    """What `gather_load` (kind "store") and `gather_load_frames` (kind "frames": ages and frame_stack are its own) share: the checks, the
    outputs, the argument list and the entry point, one-list, rows2 or (shifts with a nonzero pad) shift."""
    frames = kind == "frames"
    ref = image if image is not None else tactile
    if ref is None:
        raise ValueError(f"{who}: neither an image nor a tactile {'frame store' if frames else 'store'}")
    for name, t, nxt in (("image", image, image_next), ("tactile", tactile, tactile_next)):
        for what, x in ((f"{name}_{kind}", t), (f"{name}_next_{kind}", nxt)):
            if x is not None:
                _require_cuda(x, f"{who}: {what}")
        if nxt is not None and (t is None or nxt.shape != t.shape or nxt.dtype != t.dtype or not nxt.is_contiguous()):
            raise ValueError(f"{who}: {name}_next_{kind} must be a contiguous tensor of {name}_{kind}'{'' if frames else 's'} shape and dtype")
    _check_rows(who, rows)
    if next_rows is not None:
        _check_next_rows(who, next_rows, rows)
    if frames:
        fs = int(frame_stack)
        if fs < 1:
            raise ValueError(f"{who}: frame_stack={frame_stack}")
        T, n_envs, H, W, th, tw, S = _check_stores(who, image, tactile, frames=True)
        _require_cuda(ages, who + ": ages")
        if ages.dtype != torch.int32 or tuple(ages.shape) != (T, n_envs) or not ages.is_contiguous():
            raise ValueError(f"{who}: ages must be a contiguous int32 tensor of shape (T, n_envs) = {(T, n_envs)}")
    else:
        T, n_envs, fs, H, W, th, tw, S = _check_stores(who, image, tactile)
    B = rows.shape[0]
    image_pad, tactile_pad = _check_shift_pad(who, shift_pad)
    if shifts is not None:
        _check_shifts(who, shifts, B, ref.device)
    # a pad of a modality that is not stored shifts nothing
    shifted = shifts is not None and bool((image is not None and image_pad) or (tactile is not None and tactile_pad))
    img, tacs = _loaded_outputs(B, fs, H, W, th, tw, S, ref.device)
    img_next, tacs_next = _loaded_outputs(B, fs, H, W, th, tw, S, ref.device)
    args = (L.ptr(image), L.ptr(image_next), int(image is not None and image.dtype == torch.uint8), H, W, float(image_normalization[0]),
            float(image_normalization[1]), L.ptr(img), L.ptr(img_next), L.ptr(tactile), L.ptr(tactile_next),
            int(tactile is not None and tactile.dtype == torch.uint8), th, tw, S, float(tactile_normalization[0]), float(tactile_normalization[1]),
            L.ptr_array(tacs), L.ptr_array(tacs_next)) + ((L.ptr(ages),) if frames else ()) + (T, n_envs, fs, L.ptr(rows), int(row_shift))
    entry = "m3l_replay_gather_load" + ("_frames" if frames else "")
    if shifted:         # next_rows may be NULL there; without a shift the entry points of before run
        entry, args = entry + "_shift", args + (L.ptr(next_rows), L.ptr(shifts), image_pad, tactile_pad)
    elif next_rows is not None:
        entry, args = entry + "_rows2", args + (L.ptr(next_rows),)
    L.check(getattr(L.lib(), entry)(*args, B, _stream()), entry)
    return _as_loaded(img, tacs), _as_loaded(img_next, tacs_next)


def gather_load(image_store, tactile_store, rows, image_next_store=None, tactile_next_store=None, image_normalization=(0, 1),
                tactile_normalization=(-1, 1), row_shift=0, next_rows=None, shifts=None, shift_pad=(0, 0)):
    """image_store (T, n_envs, fs, H, W, 3) and / or tactile_store (T, n_envs, fs, 3*S, h, w), uint8 or float32 CUDA tensors, and rows (B) int64
    store rows t * n_envs + e -> (observations, next_observations), two LoadedObs {'image': (B, 3*fs, H, W), 'tactile1..S': (B, 3*fs, h, w)}:
    what `vt_load(_flatten_frame_stack(store[t, e]))` gives for both, in one launch (m3l_replay_gather_load).  The next observation is read
    from `*_next_store` at the same row, or without one from the store itself at step (t + 1) % T.
    next_rows (B) int64: the next observations are those of these store rows instead, taken as they are — row_shift applies to rows alone —
    and an entry outside [0, T n_envs) gives NaN in that half only (m3l_replay_gather_load_rows2).
    shifts (B, 2, 2, 2) int32 [sample, half, modality, (dy, dx)] with shift_pad = (image_pad, tactile_pad): the random shift of the module's
    docstring, out[y, x] = in[clamp(y + dy), clamp(x + dx)] with every shift clamped to its modality's pad, in the same one launch
    (m3l_replay_gather_load_shift).  Without shifts, or with no nonzero pad of a stored modality, the entry points above run."""
    return _gather_load("replay.gather_load", "store", image_store, tactile_store, rows, image_next_store, tactile_next_store, image_normalization,
                        tactile_normalization, row_shift, next_rows, shifts=shifts, shift_pad=shift_pad)


def gather_load_frames(image_frames, tactile_frames, ages, rows, image_next_frames=None, tactile_next_frames=None, image_normalization=(0, 1),
                       tactile_normalization=(-1, 1), row_shift=0, next_rows=None, shifts=None, shift_pad=(0, 0), *, frame_stack):
    """`gather_load` on frame-deduplicated stores: image_frames (T, n_envs, H, W, 3) and / or tactile_frames (T, n_envs, 3*S, h, w), uint8 or
    float32 CUDA tensors whose slot t holds the newest frame of step t's observation, ages (T, n_envs) int32 — how many earlier frames of the
    same episode the stack of a step reaches, clamped by the kernel to [0, frame_stack - 1] — and rows (B) int64 -> (observations,
    next_observations) as `gather_load` returns them, in one launch (m3l_replay_gather_load_frames).  Observation frame j is the frame of step
    t - min(frame_stack - 1 - j, age) in the ring; the next observation is frames 1.. of that and the frame of `*_next_frames` at the same row,
    or without one of the store itself at step (t + 1) % T.
    next_rows (B) int64: the next observations are those of these store rows instead, taken as they are, each with its own age: 2 *
    frame_stack source frames per sample, every one written once (m3l_replay_gather_load_frames_rows2); an entry outside [0, T n_envs)
    gives NaN in that half only.
    shifts, shift_pad: as for `gather_load` (m3l_replay_gather_load_frames_shift).  The two halves of a sample have shifts of their own, so
    the shifted form reads 2 * frame_stack source frames per sample with or without next_rows."""
    return _gather_load("replay.gather_load_frames", "frames", image_frames, tactile_frames, rows, image_next_frames, tactile_next_frames,
                        image_normalization, tactile_normalization, row_shift, next_rows, ages, frame_stack, shifts, shift_pad)


def _scalar_rows(who, actions, rewards, dones, timeouts, rows, reward_scale, reward_clip, row_shift, nstep=None, return_rows=True):
    """What `gather_rows` (nstep None) and `nstep_rows` (nstep = (n_steps, gamma, newest)) share: the checks, the outputs and the launch."""
    for t in (actions, rewards, dones, timeouts):
        if t is not None:
            _require_cuda(t, who + ": every argument")
    _check_rows(who, rows)
    T, n_envs, A = actions.shape
    B = rows.shape[0]
    for t in (actions, rewards, dones, timeouts):
        if t is not None and (t.dtype != torch.float32 or not t.is_contiguous() or tuple(t.shape[:2]) != (T, n_envs)):
            raise ValueError(who + ": contiguous float32 (T, n_envs, ...) tensors expected")
    dev = actions.device
    out = [torch.empty(B, A, dtype=torch.float32, device=dev)] + [torch.empty(B, 1, dtype=torch.float32, device=dev) for _ in range(2)]
    head = (L.ptr(actions), L.ptr(rewards), L.ptr(dones), L.ptr(timeouts), T, n_envs, A, L.ptr(rows), int(row_shift), B, float(reward_scale),
            float(reward_clip))
    if nstep is None:
        rows_out = [torch.empty(B, dtype=torch.int64, device=dev)] if return_rows else []
        L.check(L.lib().m3l_replay_gather_rows(*head, *[L.ptr(t) for t in out], L.ptr(rows_out[0]) if return_rows else None, _stream()),
                "m3l_replay_gather_rows")
        return tuple(out + rows_out)
    n_steps, gamma, newest = nstep
    if int(n_steps) != n_steps or not 1 <= int(n_steps) <= T:
        raise ValueError(f"{who}: n_steps={n_steps} must be an integer in [1, {T}], the steps of the ring")
    if not 0.0 < float(gamma) <= 1.0:
        raise ValueError(f"{who}: gamma={gamma} must lie in (0, 1]")
    if int(newest) != newest or not 0 <= int(newest) < T:
        raise ValueError(f"{who}: newest={newest} must be a step of the ring, in [0, {T})")
    out += [torch.empty(B, 1, dtype=torch.float32, device=dev)] + [torch.empty(B, dtype=torch.int64, device=dev) for _ in range(2)]
    L.check(L.lib().m3l_replay_nstep_rows(*head, int(n_steps), float(gamma), int(newest), *[L.ptr(t) for t in out], _stream()),
            "m3l_replay_nstep_rows")
    return tuple(out)


def gather_rows(actions, rewards, dones, timeouts, rows, reward_scale=0.0, reward_clip=0.0, row_shift=0, return_rows=False):
    """actions (T, n_envs, A) and rewards / dones / timeouts (T, n_envs) float32 CUDA tensors (timeouts may be None), rows (B) int64 ->
    actions (B, A), rewards (B, 1), dones (B, 1) in one launch (m3l_replay_gather_rows): dones * (1 - timeouts), and with reward_scale > 0
    clip(rewards / reward_scale, -reward_clip, reward_clip).  return_rows: also the (B) int64 rows read, (rows + row_shift) % (T n_envs).  A row
    outside [0, T n_envs) gives NaN and -1."""
    return _scalar_rows("replay.gather_rows", actions, rewards, dones, timeouts, rows, reward_scale, reward_clip, row_shift, None, return_rows)


def nstep_rows(actions, rewards, dones, timeouts, rows, n_steps, gamma, newest, reward_scale=0.0, reward_clip=0.0, row_shift=0):
    """`gather_rows` for n-step returns (m3l_replay_nstep_rows, one launch): from step t of every row the walk goes up to n_steps - 1 steps
    towards newer ones in the ring and ends at the first done, at step `newest` (the step written last) or after n_steps - 1 moves ->
    actions (B, A) of the rows; rewards (B, 1), the sum of gamma^k times the (normalised) rewards along the walk; dones (B, 1) of the last step,
    masked by its timeout; discounts (B, 1), gamma^(steps walked + 1); rows (B) and next_rows (B) int64, the rows of the first and the last
    step.  n_steps = 1 gives `gather_rows`' bits and discounts = float32(gamma).  A row outside [0, T n_envs) gives NaN and -1."""
    return _scalar_rows("replay.nstep_rows", actions, rewards, dones, timeouts, rows, reward_scale, reward_clip, row_shift, (n_steps, gamma, newest))


PER_BLOCK = 1024                        # M3L_PER_BLOCK: rows per block of the priority structure
PER_MAX_ROWS = PER_BLOCK * 4096         # M3L_PER_BLOCK * M3L_PER_MAX_BLOCKS: the rows whose block prefix fits the sampler's LDS
PER_MAX_UPDATE = 16384                  # M3L_PER_MAX_UPDATE: entries of one per_update


def _per_blocks(n_rows):
    return (int(n_rows) + PER_BLOCK - 1) // PER_BLOCK


def _check_per(who, mass, block_mass=None, block_min=None, max_priority=None):
    """The arrays of the priority structure -> the number of rows.  block_mass / block_min / max_priority are checked when given."""
    _require_cuda(mass, who + ": mass")
    if mass.dtype != torch.float32 or not mass.is_contiguous() or mass.numel() < 1:
        raise ValueError(f"{who}: mass must be a non-empty contiguous float32 tensor")
    n = mass.numel()
    if n > PER_MAX_ROWS:
        raise ValueError(f"{who}: {n} rows; the priority structure holds at most {PER_MAX_ROWS} (PER_BLOCK = {PER_BLOCK} rows times 4096 blocks)")
    for name, t, count in (("block_mass", block_mass, _per_blocks(n)), ("block_min", block_min, _per_blocks(n)), ("max_priority", max_priority, 1)):
        if t is not None:
            _require_cuda(t, f"{who}: {name}")
            if t.dtype != torch.float32 or not t.is_contiguous() or t.numel() != count or t.device != mass.device:
                raise ValueError(f"{who}: {name} must be a contiguous float32 tensor of {count} value(s) on mass's device")
    return n


def _check_unit(who, name, v):
    if isinstance(v, bool) or not isinstance(v, (int, float, np.floating, np.integer)) or not 0.0 <= float(v) <= 1.0:
        raise ValueError(f"{who}: {name}={v!r} must be a number in [0, 1]")
    return float(v)


def _check_eps(who, v):
    if isinstance(v, bool) or not isinstance(v, (int, float, np.floating, np.integer)) or not (float(v) > 0.0 and math.isfinite(float(v))):
        raise ValueError(f"{who}: priority_eps={v!r} must be a positive finite number")
    return float(v)


def per_refresh(mass, block_mass=None, block_min=None):
    """mass (any shape, N = T n_envs float32 values: priority^alpha per store row, 0 for a row that is not sampled) -> (block_mass, block_min),
    (ceil(N / PER_BLOCK),) each: the sum and the smallest positive leaf (+inf: none) of every block, recomputed from the leaves in one launch
    (m3l_replay_per_refresh).  block_mass / block_min: written in place when given."""
    who = "replay.per_refresh"
    n = _check_per(who, mass, block_mass, block_min)
    if block_mass is None:
        block_mass = torch.empty(_per_blocks(n), dtype=torch.float32, device=mass.device)
    if block_min is None:
        block_min = torch.empty(_per_blocks(n), dtype=torch.float32, device=mass.device)
    L.check(L.lib().m3l_replay_per_refresh(L.ptr(mass), n, L.ptr(block_mass), L.ptr(block_min), _stream()), "m3l_replay_per_refresh")
    return block_mass, block_min


def per_sample(mass, block_mass, block_min, u, beta=0.4, stratified=True, rows=None):
    """The proportional draw of prioritised replay, one launch (m3l_replay_per_sample): u (B) float32 in [0, 1) -> rows (B) int64, weights (B, 1).
    total = sum(block_mass); x_k = (k + u_k) * (total / B) if stratified, else u_k * total; the block is the first whose inclusive prefix exceeds
    x_k, the row the first leaf of that block whose inclusive prefix exceeds what is left of x_k; where rounding leaves none, the last of
    positive mass.  A row of zero mass is never returned while total > 0 (total == 0: rows -1, weights NaN).
    weights = (min positive mass / mass[row])^beta.  rows (B) int64: those rows are taken as they are (u may be None) and only their weights
    are formed; NaN for a row outside the structure or of zero mass."""
    who = "replay.per_sample"
    n = _check_per(who, mass, block_mass, block_min)
    beta = _check_unit(who, "beta", beta)
    if rows is not None:
        _check_rows(who, rows)
        B = rows.shape[0]
    if u is not None:
        _require_cuda(u, who + ": u")
        if u.dtype != torch.float32 or u.dim() != 1 or not u.is_contiguous() or (rows is not None and u.shape[0] != B):
            raise ValueError(f"{who}: u must be a contiguous 1-D float32 tensor" + (" of rows' length" if rows is not None else ""))
        B = u.shape[0]
    elif rows is None:
        raise ValueError(f"{who}: neither u nor rows")
    if B < 1:
        raise ValueError(f"{who}: an empty batch")
    out = torch.empty(B, dtype=torch.int64, device=mass.device)
    weights = torch.empty(B, 1, dtype=torch.float32, device=mass.device)
    L.check(L.lib().m3l_replay_per_sample(L.ptr(mass), L.ptr(block_mass), L.ptr(block_min), n, L.ptr(u), L.ptr(rows), B, beta, int(bool(stratified)),
                                          L.ptr(out), L.ptr(weights), _stream()), "m3l_replay_per_sample")
    return out, weights


def per_update(mass, block_mass, block_min, max_priority, rows, td, alpha=0.6, priority_eps=1e-6):
    """mass[rows[b]] = (|td[b]| + priority_eps)^alpha in place, two launches and nothing read back (m3l_replay_per_update).  rows (B) int64, td
    (B) or (B, 1) float32.  A non-finite td takes the max_priority of before the call as its priority; a row outside the structure or of zero
    mass is skipped; of duplicate rows the largest priority wins; max_priority (1) becomes the max of itself and the finite priorities that
    were applied; the blocks of the rows named are then recomputed from their leaves."""
    who = "replay.per_update"
    n = _check_per(who, mass, block_mass, block_min, max_priority)
    alpha, eps = _check_unit(who, "alpha", alpha), _check_eps(who, priority_eps)
    _check_rows(who, rows)
    _require_cuda(td, who + ": td")
    B = rows.shape[0]
    if td.dtype != torch.float32 or tuple(td.shape) not in ((B,), (B, 1)) or not td.is_contiguous():
        raise ValueError(f"{who}: td must be a contiguous float32 tensor of shape ({B},) or ({B}, 1)")
    if not 1 <= B <= PER_MAX_UPDATE:
        raise ValueError(f"{who}: {B} entries; one update takes from 1 to {PER_MAX_UPDATE} (every entry is compared with every other)")
    L.check(L.lib().m3l_replay_per_update(L.ptr(mass), L.ptr(block_mass), L.ptr(block_min), L.ptr(max_priority), n, L.ptr(rows), L.ptr(td), B, alpha,
                                          eps, _stream()), "m3l_replay_per_update")


def reward_normalization(env):
    """(scale, clip) of `VecNormalize.normalize_reward` for a duck-typed env — clip(r / sqrt(ret_rms.var + epsilon), -clip_reward, clip_reward),
    the scale formed in double and rounded to float32 once — or (0.0, 0.0) for raw rewards (env None or norm_reward false).  A few Python
    floats read on the host: no device work."""
    if env is None:
        return 0.0, 0.0
    if getattr(env, "norm_obs", False):
        raise ValueError("DeviceReplayBuffer.sample: env.norm_obs is set; observation normalisation is not covered (the reference uses "
                         "VecNormalize(norm_obs=False, norm_reward=True))")
    if not getattr(env, "norm_reward", False):
        return 0.0, 0.0
    scale = float(np.float32(math.sqrt(float(env.ret_rms.var) + float(env.epsilon))))
    clip = float(env.clip_reward)
    if not (scale > 0 and math.isfinite(scale) and clip >= 0):
        raise ValueError(f"DeviceReplayBuffer.sample: reward normalisation with scale {scale} and clip {clip}")
    return scale, clip


class ReplayBatch(NamedTuple):
    """One batch: SB3's `DictReplayBufferSamples` with both observation dicts already loaded, and the sampled rows t * n_envs + e appended."""
    observations: LoadedObs
    actions: torch.Tensor
    next_observations: LoadedObs
    dones: torch.Tensor
    rewards: torch.Tensor
    rows: torch.Tensor


class NStepReplayBatch(NamedTuple):
    """One batch of n-step returns (`DeviceReplayBuffer(n_steps > 1)`): `ReplayBatch`'s fields, where rewards are the discounted sums, dones and
    next_observations those of the last step of each walk; discounts (B, 1) = gamma^(steps walked), what `td_target` takes as `gamma`; next_rows
    (B) the rows of the last steps."""
    observations: LoadedObs
    actions: torch.Tensor
    next_observations: LoadedObs
    dones: torch.Tensor
    rewards: torch.Tensor
    rows: torch.Tensor
    discounts: torch.Tensor
    next_rows: torch.Tensor


class PrioritizedReplayBatch(NamedTuple):
    """One batch of `DeviceReplayBuffer(prioritized=True)`: `NStepReplayBatch`'s fields (with n_steps = 1: discounts = float32(gamma) and
    next_rows == rows) plus weights (B, 1), the importance weights (min mass / mass[row])^beta that `critic_loss(..., weights=)` takes.  `rows` is
    what `update_priorities` takes back."""
    observations: LoadedObs
    actions: torch.Tensor
    next_observations: LoadedObs
    dones: torch.Tensor
    rewards: torch.Tensor
    rows: torch.Tensor
    discounts: torch.Tensor
    next_rows: torch.Tensor
    weights: torch.Tensor


class DeviceReplayBuffer:
    """The surface `SAC_MAE` uses on SB3's `DictReplayBuffer` — add, sample, size, reset, pos, full — over device memory, plus the single-store
    mode of SB3's plain `ReplayBuffer` (`optimize_memory_usage`: the next observation of step t is the observation of step t + 1).

    buffer_size  transitions asked for; the capacity in steps is max(buffer_size // n_envs, 1), kept in `buffer_size` as SB3 does
    obs_shapes   {'image': (fs, H, W, 3), 'tactile': (fs, 3*S, h, w)}: the per-environment observation shapes of the vec-env, either key optional
    obs_dtypes   {'image': uint8 | float32, 'tactile': ...} (numpy or torch dtypes)
    The stores are allocated by the first add(), which first compares `store_bytes()` with the free memory of the device.

    frame_dedup     store every frame once: `frames` / `next_frames` {'image': (T, n_envs, H, W, 3), 'tactile': (T, n_envs, 3*S, h, w)} and `ages`
                    (T, n_envs) int32 stand where `observations` / `next_observations` stand without it.  add() keeps its signature and copies
                    only the newest frame of each stacked observation.  The contract: the observations are the rolling stacks of the reference's
                    FrameStack wrapper — next_obs[:, :-1] == obs[:, 1:], a constant stack at the first add() and after a `done`, otherwise obs
                    equal to the previous next_obs.  A full ring does not sample its frame_stack - 1 oldest steps, whose history the newest
                    steps overwrote (SB3 would sample them).  The capacity in steps must be at least frame_stack + 1.
    n_steps, gamma  n_steps > 1: `sample()` returns n-step returns as an `NStepReplayBatch` (the module's docstring has the rule); an integer
                    from 1 to the capacity in steps, gamma in (0, 1].  n_steps = 1 is the one-step buffer and ignores gamma.  Not with
                    optimize_memory_usage=True (SB3's rule: the single store has no agreed next observation where a walk ends).
    prioritized     proportional prioritised replay (the module's docstring has the rule): `sample()` draws rows in proportion to `mass` and
                    returns a `PrioritizedReplayBatch`, `update_priorities(rows, td_errors)` writes the new priorities.  alpha in [0, 1] is the
                    exponent of the priorities, beta in [0, 1] the default exponent of the weights (`sample(beta=)` overrides it), priority_eps
                    > 0 is added to |td|.  `mass` (T, n_envs), `block_mass`, `block_min` and `max_priority` (1) live on the device; at most
                    PER_MAX_ROWS = 2^22 transitions.  With every combination of frame_dedup, n_steps and optimize_memory_usage that is allowed
                    without it.  False: the buffer has none of these arrays and launches none of these kernels.
    random_shift    the random-shift augmentation of both observation dicts (the module's docstring has the rule): None is off — no new array, no
                    new launch, the entry points of before — an integer p pads both modalities by p, dict(image=p_i, tactile=p_t) sets them
                    separately (a missing key: 0); all pads 0 is None.  `sample()` draws the shifts on the device, or takes `shifts=`, and keeps
                    the tensor it used in `last_shifts`.  A pad must be an integer in [0, 2^15), and 0 for a modality that is not stored.
    check_stacking  with frame_dedup: every add() verifies that contract with torch ops on the device and one read-back — it synchronises: for
                    tests and a first run — and raises ValueError naming the key, the environment and the rule.
    """

    def __init__(self, buffer_size, n_envs, obs_shapes, obs_dtypes, action_dim, optimize_memory_usage=False, handle_timeout_termination=True,
                 image_normalization=[0, 1], tactile_normalization=[-1, 1], device="cuda", frame_dedup=False, check_stacking=False, n_steps=1, gamma=0.99,
                 prioritized=False, alpha=0.6, beta=0.4, priority_eps=1e-6, random_shift=None):
        self.device = _require_device("DeviceReplayBuffer", device, "replay buffer", "DictReplayBuffer")
        self.n_envs, self.action_dim = int(n_envs), int(action_dim)
        if int(buffer_size) < 1 or self.n_envs < 1 or self.action_dim < 1:
            raise ValueError(f"DeviceReplayBuffer: buffer_size={buffer_size}, n_envs={n_envs}, action_dim={action_dim} must be positive")
        self.buffer_size = max(int(buffer_size) // self.n_envs, 1)
        self.obs_shapes, self.obs_dtypes, self.frame_stack = _obs_spec("DeviceReplayBuffer", obs_shapes, obs_dtypes, image_normalization,
                                                                       tactile_normalization)
        self.optimize_memory_usage, self.handle_timeout_termination = bool(optimize_memory_usage), bool(handle_timeout_termination)
        if self.optimize_memory_usage and self.handle_timeout_termination:
            raise ValueError("DeviceReplayBuffer: optimize_memory_usage=True needs handle_timeout_termination=False (the single store loses the "
                             "true next observation of a truncated step)")
        self.image_normalization, self.tactile_normalization = list(image_normalization), list(tactile_normalization)
        self.frame_dedup, self.check_stacking = bool(frame_dedup), bool(check_stacking)
        if self.check_stacking and not self.frame_dedup:
            raise ValueError("DeviceReplayBuffer: check_stacking=True checks the contract of frame_dedup=True and needs it")
        if self.frame_dedup and self.buffer_size < self.frame_stack + 1:
            raise ValueError(f"DeviceReplayBuffer: frame_dedup=True with frame_stack={self.frame_stack} needs a capacity of at least "
                             f"{self.frame_stack + 1} steps (buffer_size // n_envs is {self.buffer_size})")
        if isinstance(n_steps, bool) or not isinstance(n_steps, (int, np.integer)) or not 1 <= int(n_steps) <= self.buffer_size:
            raise ValueError(f"DeviceReplayBuffer: n_steps={n_steps!r} must be an integer from 1 to the capacity in steps ({self.buffer_size})")
        if isinstance(gamma, bool) or not isinstance(gamma, (int, float, np.floating)) or not 0.0 < float(gamma) <= 1.0:
            raise ValueError(f"DeviceReplayBuffer: gamma={gamma!r} must be a number in (0, 1]")
        self.n_steps, self.gamma = int(n_steps), float(gamma)
        if self.n_steps > 1 and self.optimize_memory_usage:
            raise ValueError("DeviceReplayBuffer: n_steps > 1 needs optimize_memory_usage=False (the single store has no agreed next observation at "
                             "the step where a walk ends: the slot after it holds the next episode's reset stack or the ring's oldest step)")
        self.prioritized = bool(prioritized)
        self.alpha, self.beta = _check_unit("DeviceReplayBuffer", "alpha", alpha), _check_unit("DeviceReplayBuffer", "beta", beta)
        self.priority_eps = _check_eps("DeviceReplayBuffer", priority_eps)
        if self.prioritized and self.buffer_size * self.n_envs > PER_MAX_ROWS:
            raise ValueError(f"DeviceReplayBuffer: prioritized=True holds at most {PER_MAX_ROWS} transitions (PER_BLOCK = {PER_BLOCK} rows times 4096 "
                             f"blocks, the block prefix a sample keeps on chip); {self.buffer_size} steps of {self.n_envs} environments are "
                             f"{self.buffer_size * self.n_envs}")
        self.random_shift = _shift_pads("DeviceReplayBuffer: random_shift", random_shift, self.obs_shapes)      # None, or (image_pad, tactile_pad)
        self.last_shifts = None
        self.observations = self.next_observations = None
        self.frames = self.next_frames = self.ages = None
        self.mass = self.block_mass = self.block_min = self.max_priority = None
        self.reset()

    # ---- memory
    def _store_bytes(self, frame_dedup):
        shapes = {k: s[1:] for k, s in self.obs_shapes.items()} if frame_dedup else self.obs_shapes
        per_step = sum(int(np.prod(s)) * torch.empty(0, dtype=self.obs_dtypes[k]).element_size() for k, s in shapes.items()) * self.n_envs
        obs = per_step * self.buffer_size
        nxt = 0 if self.optimize_memory_usage else obs
        scalars = 4 * self.buffer_size * self.n_envs * (self.action_dim + 2 + int(self.handle_timeout_termination) + int(frame_dedup))
        if self.prioritized:        # mass, block_mass, block_min, max_priority
            scalars += 4 * (self.buffer_size * self.n_envs + 2 * _per_blocks(self.buffer_size * self.n_envs) + 1)
        return {"observations": obs, "next_observations": nxt, "scalars": scalars, "total": obs + nxt + scalars}

    def store_bytes(self):
        """Bytes of the stores, before or after allocation: {'observations', 'next_observations' (0 in the single-store mode), 'scalars', 'total'}.
        With frame_dedup the first two are the frame stores and 'scalars' counts the 4 bytes per (step, environment) of `ages`; with prioritized
        it counts `mass`, `block_mass`, `block_min` and `max_priority`."""
        return self._store_bytes(self.frame_dedup)

    def _allocate(self):
        need = self.store_bytes()["total"]
        free = torch.cuda.mem_get_info(self.device)[0]
        free += torch.cuda.memory_reserved(self.device) - torch.cuda.memory_allocated(self.device)      # blocks torch holds and can reuse
        if need > free:
            dedup = ""
            if not self.frame_dedup and self.frame_stack > 1:
                n = self._store_bytes(True)["total"]
                dedup = f", or frame_dedup=True (every frame of the frame stack stored once: {n} B, {n / 1e9:.1f} GB)"
            raise L.M3LError(f"DeviceReplayBuffer: the stores need {need} bytes ({need / 1e9:.1f} GB) and {free} bytes ({free / 1e9:.1f} GB) of "
                             f"device memory are free; ways out: uint8 stores (obs_dtypes), optimize_memory_usage=True (one observation store "
                             f"instead of two), or a smaller buffer_size (now {self.buffer_size} steps of {self.n_envs} environments){dedup}")
        T, E, dev = self.buffer_size, self.n_envs, self.device
        shapes = {k: s[1:] for k, s in self.obs_shapes.items()} if self.frame_dedup else self.obs_shapes
        stores = {k: torch.empty((T, E) + s, dtype=self.obs_dtypes[k], device=dev) for k, s in shapes.items()}
        second = None if self.optimize_memory_usage else {k: torch.empty((T, E) + s, dtype=self.obs_dtypes[k], device=dev) for k, s in shapes.items()}
        if self.frame_dedup:
            self.frames, self.next_frames = stores, second
            self.ages = torch.empty(T, E, dtype=torch.int32, device=dev)
        else:
            self.observations, self.next_observations = stores, second
        self.actions = torch.empty(T, E, self.action_dim, dtype=torch.float32, device=dev)
        self.rewards = torch.empty(T, E, dtype=torch.float32, device=dev)
        self.dones = torch.empty(T, E, dtype=torch.float32, device=dev)
        self.timeouts = torch.empty(T, E, dtype=torch.float32, device=dev) if self.handle_timeout_termination else None
        if self.prioritized:
            self.mass = torch.zeros(T, E, dtype=torch.float32, device=dev)
            self.block_mass = torch.empty(_per_blocks(T * E), dtype=torch.float32, device=dev)
            self.block_min = torch.empty(_per_blocks(T * E), dtype=torch.float32, device=dev)
            self.max_priority = torch.ones(1, dtype=torch.float32, device=dev)
            per_refresh(self.mass, self.block_mass, self.block_min)

    # ---- filling
    def reset(self):
        self.pos, self.full = 0, False
        # frame_dedup, per environment on the host: the age of the last stored step, and whether the next add() starts an episode
        self._age = np.zeros(self.n_envs, dtype=np.int32)
        self._episode_start = np.ones(self.n_envs, dtype=bool)
        self._last_next_obs = None
        if self.mass is not None:           # prioritized: no row can be sampled, max_priority back to 1
            self.mass.zero_()
            per_refresh(self.mass, self.block_mass, self.block_min)
            self.max_priority.fill_(1.0)

    def size(self):
        return self.buffer_size if self.full else self.pos

    def add(self, obs, next_obs, action, reward, done, infos):
        """One vec-env step into slot `pos`: every array with one copy straight into its place, cast to the store's dtype.  In the single-store
        mode next_obs goes to slot (pos + 1) % buffer_size of `observations`, where the next add() writes the same frames again.  With
        frame_dedup the same full stacked dicts are taken and only their newest frames are copied (`_add_frames`)."""
        _check_obs("DeviceReplayBuffer.add", obs, self.obs_shapes, self.n_envs)
        _check_obs("DeviceReplayBuffer.add (next_obs)", next_obs, self.obs_shapes, self.n_envs)
        if self.handle_timeout_termination and len(infos) != self.n_envs:
            raise ValueError(f"DeviceReplayBuffer.add: {len(infos)} infos for {self.n_envs} environments")
        if (self.frames if self.frame_dedup else self.observations) is None:
            self._allocate()
        p, T = self.pos, self.buffer_size
        if self.frame_dedup:
            self._add_frames(obs, next_obs, done)
        else:
            for k in self.obs_shapes:
                self.observations[k][p].copy_(torch.as_tensor(obs[k]))
                nxt = self.observations[k][(p + 1) % T] if self.optimize_memory_usage else self.next_observations[k][p]
                nxt.copy_(torch.as_tensor(next_obs[k]))
        self.actions[p].copy_(torch.as_tensor(action).reshape(self.n_envs, self.action_dim))
        self.rewards[p].copy_(torch.as_tensor(reward).reshape(self.n_envs))
        self.dones[p].copy_(torch.as_tensor(done).reshape(self.n_envs))
        if self.handle_timeout_termination:
            self.timeouts[p].copy_(torch.tensor([float(bool(info.get("TimeLimit.truncated", False))) for info in infos], dtype=torch.float32))
        self.pos += 1
        if self.pos == T:
            self.full, self.pos = True, 0
        if self.prioritized:
            self._add_priorities(p)

    def _add_priorities(self, p):
        """prioritized: the step just written takes max_priority^alpha in every environment, and the steps after it that a full ring does not
        sample (`_valid_steps`: the slot the newest next observation lies in, the frame_stack - 1 steps whose history is gone) take 0 — they
        follow step p in the ring, so it is one range of rows — then the blocks that range touches are recomputed (m3l_replay_per_add: two
        launches)."""
        n_zero = self._skipped_steps() * self.n_envs if self.full else 0
        L.check(L.lib().m3l_replay_per_add(L.ptr(self.mass), L.ptr(self.block_mass), L.ptr(self.block_min), L.ptr(self.max_priority),
                                           self.buffer_size * self.n_envs, p * self.n_envs, self.n_envs, n_zero, self.alpha, _stream()),
                "m3l_replay_per_add")

    _STACKING_RULES = ("next_obs[:, :-1] == obs[:, 1:]", "all frames of obs are equal at an episode's first step",
                       "obs equals the previous add()'s next_obs")

    def _add_frames(self, obs, next_obs, done):
        """frame_dedup: the newest frame of each stacked observation into its slot — in the single-store mode next_obs's into slot (pos + 1) %
        buffer_size of `frames`, where the next add() writes the same frame again — and the step's ages, kept per environment on the host."""
        d = torch.as_tensor(done).reshape(self.n_envs)
        if d.is_cuda:
            raise ValueError("DeviceReplayBuffer.add: frame_dedup=True follows the episodes on the host and needs `done` there")
        age = np.where(self._episode_start, 0, np.minimum(self._age + 1, self.frame_stack - 1)).astype(np.int32)
        checked = self._check_stacking(obs, next_obs, age) if self.check_stacking else None
        p, T = self.pos, self.buffer_size
        for k in self.obs_shapes:
            self.frames[k][p].copy_(torch.as_tensor(obs[k])[:, -1])
            nxt = self.frames[k][(p + 1) % T] if self.optimize_memory_usage else self.next_frames[k][p]
            nxt.copy_(torch.as_tensor(next_obs[k])[:, -1])
        self.ages[p].copy_(torch.from_numpy(age))
        self._age, self._episode_start, self._last_next_obs = age, d.numpy().astype(bool), checked

    def _check_stacking(self, obs, next_obs, age):
        """The stacking contract of this add() on the device, with one read-back -> next_obs on the device, for the next add()'s check."""
        start = torch.from_numpy(age == 0).to(self.device)
        rows = lambda x: x.reshape(self.n_envs, -1)      # noqa: E731
        flags, cur = [], {}
        for k in self.obs_shapes:
            o, n = torch.as_tensor(obs[k]).to(self.device), torch.as_tensor(next_obs[k]).to(self.device)
            shifted = (rows(n[:, :-1]) == rows(o[:, 1:])).all(1)
            constant = (rows(o[:, 1:]) == rows(o[:, :-1])).all(1) | ~start
            follows = torch.ones_like(start) if self._last_next_obs is None else (rows(o) == rows(self._last_next_obs[k])).all(1) | start
            flags.append(torch.stack([shifted, constant, follows]))
            cur[k] = n
        ok = torch.stack(flags).cpu().numpy()
        for i, k in enumerate(self.obs_shapes):
            for r, rule in enumerate(self._STACKING_RULES):
                if not ok[i, r].all():
                    e = int(np.flatnonzero(~ok[i, r])[0])
                    raise ValueError(f"DeviceReplayBuffer.add: check_stacking: observation '{k}' of environment {e} breaks the contract of "
                                     f"frame_dedup=True: {rule} (the stack reaches {int(age[e])} earlier frames of its episode)")
        return cur

    # ---- sampling
    def _skipped_steps(self):
        """The oldest steps that a full ring does not sample: step `pos` in the single-store mode — the newest next observation lies there —
        and with frame_dedup the frame_stack - 1 steps after it, whose stacks reach frames that the newest steps overwrote."""
        return int(self.optimize_memory_usage) + (self.frame_stack - 1 if self.frame_dedup else 0)

    def _valid_steps(self):
        """The steps a sample may come from, as (first, count) in the ring: count steps starting at `first`, modulo buffer_size: all that were
        written but a full ring's `_skipped_steps()`."""
        skip = self._skipped_steps()
        if self.full and skip:
            return (self.pos + skip) % self.buffer_size, self.buffer_size - skip
        return 0, self.size()

    def _injected(self, indices):
        """(batch_inds, env_indices) checked on the host — the kernels cannot report a wrong row — -> rows t * n_envs + e on the device."""
        try:
            t, e = (torch.as_tensor(x).detach().cpu() for x in indices)
        except (TypeError, ValueError):
            raise ValueError("DeviceReplayBuffer.sample: indices must be a pair (batch_inds, env_indices)") from None
        ints = (torch.int64, torch.int32)
        if t.dim() != 1 or e.dim() != 1 or t.dtype not in ints or e.dtype not in ints or t.numel() == 0 or t.shape != e.shape:
            raise ValueError("DeviceReplayBuffer.sample: indices must be two non-empty 1-D integer sequences of one length")
        t, e = t.to(torch.int64), e.to(torch.int64)
        first, count = self._valid_steps()
        T = self.buffer_size
        if int(t.min()) < 0 or int(t.max()) >= T or int(((t - first) % T).max()) >= count:
            raise ValueError(f"DeviceReplayBuffer.sample: indices name steps outside the {count} valid ones (from step {first}, ring of {T})")
        if int(e.min()) < 0 or int(e.max()) >= self.n_envs:
            raise ValueError(f"DeviceReplayBuffer.sample: indices name environments outside [0, {self.n_envs})")
        return (t * self.n_envs + e).to(self.device)

    def _check_injected_shifts(self, shifts, batch_size, indices, u):
        """`sample(shifts=)` checked before anything is launched: it belongs to random_shift and has one entry per sample."""
        who = "DeviceReplayBuffer.sample"
        if self.random_shift is None:
            raise ValueError(f"{who}: shifts= belongs to a buffer built with random_shift")
        if indices is not None:
            try:
                B = len(indices[0])
            except (TypeError, IndexError):
                raise ValueError(f"{who}: indices must be a pair (batch_inds, env_indices)") from None
        else:
            B = int(u.shape[0]) if isinstance(u, torch.Tensor) and u.dim() == 1 else int(batch_size)
        _check_shifts(who, shifts, B)

    def sample(self, batch_size, env=None, indices=None, beta=None, u=None, shifts=None):
        """`batch_size` transitions drawn uniformly over the valid (step, environment) pairs with one torch.randint on the device (nothing is
        read back), or the pairs of `indices` = (batch_inds, env_indices).  env: a VecNormalize-like object whose reward normalisation is
        applied (`norm_reward`, `ret_rms.var`, `epsilon`, `clip_reward`), or None for raw rewards.  With n_steps > 1 the batch is an
        `NStepReplayBatch`: still three launches — the draw, `nstep_rows`, one gather fed rows and next_rows — and nothing read back.
        prioritized: the rows are drawn in proportion to `mass` from u, `batch_size` uniform numbers of one torch.rand on the device or the
        injected float32 tensor `u` (the parity seam), with weights of exponent `beta` (None: the buffer's) — four launches: the draw,
        `per_sample`, `nstep_rows`, the gather — and the batch is a `PrioritizedReplayBatch`; with `indices` the rows are those and the
        weights are still formed.
        random_shift: both observation dicts leave the same gather launch augmented, with the shifts of one torch.randint per distinct nonzero
        pad on the device or the injected int32 tensor `shifts` (B, 2, 2, 2) (the parity seam; zeros: the unaugmented batch); the tensor used
        is kept in `last_shifts`.  The batch types and everything but the two observation dicts are as without it."""
        if not self.prioritized and (beta is not None or u is not None):
            raise ValueError("DeviceReplayBuffer.sample: beta= and u= belong to prioritized=True")
        if shifts is not None:
            self._check_injected_shifts(shifts, batch_size, indices, u)
        scale, clip = reward_normalization(env)
        first, count = self._valid_steps()
        if count < 1:
            raise ValueError("DeviceReplayBuffer.sample: the buffer is empty" if self.size() == 0 else
                             "DeviceReplayBuffer.sample: a full single-store buffer of one step holds no transition")
        weights = None
        if self.prioritized:
            draw, weights = self._draw_prioritized(batch_size, indices, beta, u)
            shift = 0
        elif indices is not None:
            draw, shift = self._injected(indices), 0
        else:
            if int(batch_size) < 1:
                raise ValueError(f"DeviceReplayBuffer.sample: batch_size={batch_size}")
            # rows relative to the first valid step; the kernels add `shift` modulo T n_envs
            draw, shift = torch.randint(0, count * self.n_envs, (int(batch_size),), device=self.device), first * self.n_envs
        if self.prioritized or self.n_steps > 1:
            newest = (self.pos - 1) % self.buffer_size
            actions, rewards, dones, discounts, rows, next_rows = nstep_rows(self.actions, self.rewards, self.dones, self.timeouts, draw, self.n_steps,
                                                                             self.gamma, newest, scale, clip, shift)
        else:
            actions, rewards, dones, rows = gather_rows(self.actions, self.rewards, self.dones, self.timeouts, draw, scale, clip, shift, return_rows=True)
        # n_steps = 1: next_rows == rows where there are any, and the one-list gathers run
        if self.random_shift is not None:
            if shifts is None:
                shifts = _draw_shifts(self.random_shift, (draw.shape[0], 2, 2, 2), self.device)
            else:
                _check_shifts("DeviceReplayBuffer.sample", shifts, draw.shape[0])
            self.last_shifts = shifts
        obs, next_obs = self._gather(draw, shift, next_rows if self.n_steps > 1 else None, shifts)
        if self.prioritized:
            return PrioritizedReplayBatch(obs, actions, next_obs, dones, rewards, rows, discounts, next_rows, weights)
        if self.n_steps > 1:
            return NStepReplayBatch(obs, actions, next_obs, dones, rewards, rows, discounts, next_rows)
        return ReplayBatch(obs, actions, next_obs, dones, rewards, rows)

    def _gather(self, rows, shift, next_rows, shifts=None):
        """(observations, next_observations) of rows (+ shift in the ring) from the frame or the stacked stores, in one launch; next_rows: the
        next observations are those rows' (n-step returns), else None; shifts: the random shifts of a random_shift buffer, else None."""
        aug = {} if shifts is None else dict(shifts=shifts, shift_pad=self.random_shift)
        if self.frame_dedup:
            nxt = self.next_frames or {}
            return gather_load_frames(self.frames.get("image"), self.frames.get("tactile"), self.ages, rows, nxt.get("image"), nxt.get("tactile"),
                                      self.image_normalization, self.tactile_normalization, shift, next_rows, frame_stack=self.frame_stack, **aug)
        nxt = self.next_observations or {}
        return gather_load(self.observations.get("image"), self.observations.get("tactile"), rows, nxt.get("image"), nxt.get("tactile"),
                           self.image_normalization, self.tactile_normalization, shift, next_rows, **aug)

    # ---- prioritised replay
    def _draw_prioritized(self, batch_size, indices, beta, u):
        """-> (rows, weights): the rows of `indices`, or drawn in proportion to `mass` from u (None: one torch.rand), and their weights."""
        beta = self.beta if beta is None else _check_unit("DeviceReplayBuffer.sample", "beta", beta)
        if indices is not None:
            if u is not None:
                raise ValueError("DeviceReplayBuffer.sample: indices and u both name the rows")
            return per_sample(self.mass, self.block_mass, self.block_min, None, beta, rows=self._injected(indices))
        if u is None:
            if int(batch_size) < 1:
                raise ValueError(f"DeviceReplayBuffer.sample: batch_size={batch_size}")
            u = torch.rand(int(batch_size), dtype=torch.float32, device=self.device)
        return per_sample(self.mass, self.block_mass, self.block_min, u, beta)

    def update_priorities(self, rows, td_errors):
        """The priorities of the sampled `rows` (B) int64 from their TD errors (B,) or (B, 1), float32 on the device (`per_update`, two launches,
        nothing read back): the batch's `rows` and the td errors that `critic_loss(..., return_td_errors=True)` returns."""
        if not self.prioritized:
            raise ValueError("DeviceReplayBuffer.update_priorities: the buffer was built without prioritized=True")
        if self.mass is None:
            raise ValueError("DeviceReplayBuffer.update_priorities: the buffer is empty")
        per_update(self.mass, self.block_mass, self.block_min, self.max_priority, rows, td_errors, self.alpha, self.priority_eps)
