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
n-step returns, HER, prioritised sampling, a frame-deduplicated store, observation normalisation (`norm_obs`).
"""
import math
from typing import NamedTuple

import numpy as np
import torch

from . import _lib as L
from .functional import _require_cuda
from .pretrain_utils import LoadedObs
from .rollout import _as_loaded, _check_obs, _check_stores, _loaded_outputs, _obs_spec, _require_device, _stream


def _check_rows(who, rows):
    _require_cuda(rows, who + ": rows")
    if rows.dtype != torch.int64 or rows.dim() != 1 or not rows.is_contiguous():
        raise ValueError(f"{who}: rows must be a contiguous 1-D int64 tensor")


def gather_load(image_store, tactile_store, rows, image_next_store=None, tactile_next_store=None, image_normalization=(0, 1),
                tactile_normalization=(-1, 1), row_shift=0):
    """image_store (T, n_envs, fs, H, W, 3) and / or tactile_store (T, n_envs, fs, 3*S, h, w), uint8 or float32 CUDA tensors, and rows (B) int64
    store rows t * n_envs + e -> (observations, next_observations), two LoadedObs {'image': (B, 3*fs, H, W), 'tactile1..S': (B, 3*fs, h, w)}:
    what `vt_load(_flatten_frame_stack(store[t, e]))` gives for both, in one launch (m3l_replay_gather_load).  The next observation is read
    from `*_next_store` at the same row, or without one from the store itself at step (t + 1) % T."""
    ref = image_store if image_store is not None else tactile_store
    if ref is None:
        raise ValueError("replay.gather_load: neither an image nor a tactile store")
    pairs = (("image", image_store, image_next_store), ("tactile", tactile_store, tactile_next_store))
    for name, t, nxt in pairs:
        for what, x in ((name + "_store", t), (name + "_next_store", nxt)):
            if x is not None:
                _require_cuda(x, "replay.gather_load: " + what)
        if nxt is not None and (t is None or nxt.shape != t.shape or nxt.dtype != t.dtype or not nxt.is_contiguous()):
            raise ValueError(f"replay.gather_load: {name}_next_store must be a contiguous tensor of {name}_store's shape and dtype")
    _check_rows("replay.gather_load", rows)
    T, n_envs, fs, H, W, th, tw, S = _check_stores("replay.gather_load", image_store, tactile_store)
    B = rows.shape[0]
    img, tacs = _loaded_outputs(B, fs, H, W, th, tw, S, ref.device)
    img_next, tacs_next = _loaded_outputs(B, fs, H, W, th, tw, S, ref.device)
    L.check(L.lib().m3l_replay_gather_load(
        L.ptr(image_store), L.ptr(image_next_store), int(image_store is not None and image_store.dtype == torch.uint8), H, W,
        float(image_normalization[0]), float(image_normalization[1]), L.ptr(img), L.ptr(img_next), L.ptr(tactile_store), L.ptr(tactile_next_store),
        int(tactile_store is not None and tactile_store.dtype == torch.uint8), th, tw, S, float(tactile_normalization[0]),
        float(tactile_normalization[1]), L.ptr_array(tacs), L.ptr_array(tacs_next), T, n_envs, fs, L.ptr(rows), int(row_shift), B, _stream()),
        "m3l_replay_gather_load")
    return _as_loaded(img, tacs), _as_loaded(img_next, tacs_next)


def gather_rows(actions, rewards, dones, timeouts, rows, reward_scale=0.0, reward_clip=0.0, row_shift=0, return_rows=False):
    """actions (T, n_envs, A) and rewards / dones / timeouts (T, n_envs) float32 CUDA tensors (timeouts may be None), rows (B) int64 ->
    actions (B, A), rewards (B, 1), dones (B, 1) in one launch (m3l_replay_gather_rows): dones * (1 - timeouts), and with reward_scale > 0
    clip(rewards / reward_scale, -reward_clip, reward_clip).  return_rows: also the (B) int64 rows read, (rows + row_shift) % (T n_envs)."""
    for t in (actions, rewards, dones, timeouts):
        if t is not None:
            _require_cuda(t, "replay.gather_rows: every argument")
    _check_rows("replay.gather_rows", rows)
    T, n_envs, A = actions.shape
    B = rows.shape[0]
    for t in (actions, rewards, dones, timeouts):
        if t is not None and (t.dtype != torch.float32 or not t.is_contiguous() or tuple(t.shape[:2]) != (T, n_envs)):
            raise ValueError("replay.gather_rows: contiguous float32 (T, n_envs, ...) tensors expected")
    dev = actions.device
    out = [torch.empty(B, A, dtype=torch.float32, device=dev), torch.empty(B, 1, dtype=torch.float32, device=dev),
           torch.empty(B, 1, dtype=torch.float32, device=dev)]
    rows_out = torch.empty(B, dtype=torch.int64, device=dev) if return_rows else None
    L.check(L.lib().m3l_replay_gather_rows(L.ptr(actions), L.ptr(rewards), L.ptr(dones), L.ptr(timeouts), T, n_envs, A, L.ptr(rows), int(row_shift), B,
                                           float(reward_scale), float(reward_clip), *[L.ptr(t) for t in out], L.ptr(rows_out), _stream()),
            "m3l_replay_gather_rows")
    return tuple(out) + ((rows_out,) if return_rows else ())


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


class DeviceReplayBuffer:
    """The surface `SAC_MAE` uses on SB3's `DictReplayBuffer` — add, sample, size, reset, pos, full — over device memory, plus the single-store
    mode of SB3's plain `ReplayBuffer` (`optimize_memory_usage`: the next observation of step t is the observation of step t + 1).

    buffer_size  transitions asked for; the capacity in steps is max(buffer_size // n_envs, 1), kept in `buffer_size` as SB3 does
    obs_shapes   {'image': (fs, H, W, 3), 'tactile': (fs, 3*S, h, w)}: the per-environment observation shapes of the vec-env, either key optional
    obs_dtypes   {'image': uint8 | float32, 'tactile': ...} (numpy or torch dtypes)
    The stores are allocated by the first add(), which first compares `store_bytes()` with the free memory of the device.
    """

    def __init__(self, buffer_size, n_envs, obs_shapes, obs_dtypes, action_dim, optimize_memory_usage=False, handle_timeout_termination=True,
                 image_normalization=[0, 1], tactile_normalization=[-1, 1], device="cuda"):
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
        self.observations = self.next_observations = None
        self.reset()

    # ---- memory
    def store_bytes(self):
        """Bytes of the stores, before or after allocation: {'observations', 'next_observations' (0 in the single-store mode), 'scalars', 'total'}."""
        per_step = sum(int(np.prod(s)) * torch.empty(0, dtype=self.obs_dtypes[k]).element_size() for k, s in self.obs_shapes.items()) * self.n_envs
        obs = per_step * self.buffer_size
        nxt = 0 if self.optimize_memory_usage else obs
        scalars = 4 * self.buffer_size * self.n_envs * (self.action_dim + 2 + int(self.handle_timeout_termination))
        return {"observations": obs, "next_observations": nxt, "scalars": scalars, "total": obs + nxt + scalars}

    def _allocate(self):
        need = self.store_bytes()["total"]
        free = torch.cuda.mem_get_info(self.device)[0]
        free += torch.cuda.memory_reserved(self.device) - torch.cuda.memory_allocated(self.device)      # blocks torch holds and can reuse
        if need > free:
            raise L.M3LError(f"DeviceReplayBuffer: the stores need {need} bytes ({need / 1e9:.1f} GB) and {free} bytes ({free / 1e9:.1f} GB) of "
                             f"device memory are free; ways out: uint8 stores (obs_dtypes), optimize_memory_usage=True (one observation store "
                             f"instead of two), or a smaller buffer_size (now {self.buffer_size} steps of {self.n_envs} environments)")
        T, E, dev = self.buffer_size, self.n_envs, self.device
        self.observations = {k: torch.empty((T, E) + s, dtype=self.obs_dtypes[k], device=dev) for k, s in self.obs_shapes.items()}
        if not self.optimize_memory_usage:
            self.next_observations = {k: torch.empty((T, E) + s, dtype=self.obs_dtypes[k], device=dev) for k, s in self.obs_shapes.items()}
        self.actions = torch.empty(T, E, self.action_dim, dtype=torch.float32, device=dev)
        self.rewards = torch.empty(T, E, dtype=torch.float32, device=dev)
        self.dones = torch.empty(T, E, dtype=torch.float32, device=dev)
        self.timeouts = torch.empty(T, E, dtype=torch.float32, device=dev) if self.handle_timeout_termination else None

    # ---- filling
    def reset(self):
        self.pos, self.full = 0, False

    def size(self):
        return self.buffer_size if self.full else self.pos

    def add(self, obs, next_obs, action, reward, done, infos):
        """One vec-env step into slot `pos`: every array with one copy straight into its place, cast to the store's dtype.  In the single-store
        mode next_obs goes to slot (pos + 1) % buffer_size of `observations`, where the next add() writes the same frames again."""
        _check_obs("DeviceReplayBuffer.add", obs, self.obs_shapes, self.n_envs)
        _check_obs("DeviceReplayBuffer.add (next_obs)", next_obs, self.obs_shapes, self.n_envs)
        if self.handle_timeout_termination and len(infos) != self.n_envs:
            raise ValueError(f"DeviceReplayBuffer.add: {len(infos)} infos for {self.n_envs} environments")
        if self.observations is None:
            self._allocate()
        p, T = self.pos, self.buffer_size
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

    # ---- sampling
    def _valid_steps(self):
        """The steps a sample may come from, as (first, count) in the ring: count steps starting at `first`, modulo buffer_size."""
        if self.optimize_memory_usage and self.full:
            return (self.pos + 1) % self.buffer_size, self.buffer_size - 1      # every step but `pos`: the newest next observation lies there
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

    def sample(self, batch_size, env=None, indices=None):
        """`batch_size` transitions drawn uniformly over the valid (step, environment) pairs with one torch.randint on the device (nothing is
        read back), or the pairs of `indices` = (batch_inds, env_indices).  env: a VecNormalize-like object whose reward normalisation is
        applied (`norm_reward`, `ret_rms.var`, `epsilon`, `clip_reward`), or None for raw rewards."""
        scale, clip = reward_normalization(env)
        first, count = self._valid_steps()
        if count < 1:
            raise ValueError("DeviceReplayBuffer.sample: the buffer is empty" if self.size() == 0 else
                             "DeviceReplayBuffer.sample: a full single-store buffer of one step holds no transition")
        if indices is not None:
            draw, shift = self._injected(indices), 0
        else:
            if int(batch_size) < 1:
                raise ValueError(f"DeviceReplayBuffer.sample: batch_size={batch_size}")
            # rows relative to the first valid step; the kernels add `shift` modulo T n_envs
            draw, shift = torch.randint(0, count * self.n_envs, (int(batch_size),), device=self.device), first * self.n_envs
        nxt = self.next_observations or {}
        obs, next_obs = gather_load(self.observations.get("image"), self.observations.get("tactile"), draw, nxt.get("image"), nxt.get("tactile"),
                                    self.image_normalization, self.tactile_normalization, shift)
        actions, rewards, dones, rows = gather_rows(self.actions, self.rewards, self.dones, self.timeouts, draw, scale, clip, shift, return_rows=True)
        return ReplayBatch(obs, actions, next_obs, dones, rewards, rows)
