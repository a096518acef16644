"""The PPO rollout kept on the GPU: `DeviceRolloutBuffer` stands where `PPO_MAE` uses SB3's `DictRolloutBuffer`, and a minibatch leaves it as
the MAE's input tensors after two launches (csrc/rollout.hip, include/m3l_amd.h "device-resident rollout").

Reference path replaced, per minibatch (models/ppo_dino_cat_mae.py): `swap_and_flatten` of every array (:25-29, :39-46), `obs[idx]` on the host
(:48-56), the DataLoader's collate and pinned upload (:268-278, :58-70), the frame-stack permute / reshape (:295-301) and `vt_load` (:320) — and
the second `vt_load` of the same rows inside the features extractor (`policy.evaluate_actions`, :343).  Here

    for batch in buffer.get(batch_size):          # batch.x: a LoadedObs = {'image', 'tactile1', ...} in the MAE's layout
        mae_loss = mae(batch.x)
        features = extractor(batch.x)             # MAEExtractor / DinoCatMAEExtractor take a LoadedObs as it is: one load feeds both

the stores keep the layout the vec-env fills them in, (T, n_envs, ...); nothing is swapped in memory.  A flat index j means what it means after
the reference's swap: env = j // T, t = j % T.  `get(indices=...)` is the parity seam (what `mask_noise=` is for the MAE): with the reference's
permutation it yields the reference's minibatches, bit for bit.

SB3's own buffer arithmetic (`RolloutBuffer.compute_returns_and_advantage`) is not in the reference tree; it is restated in csrc/rollout.hip
and, in float64, in tests/rollout_cases.py (parity unpinned).  Not covered: VecNormalize of observations, discrete action spaces.  SAC's
replay buffer is m3l_amd.replay.DeviceReplayBuffer, which shares this module's validation and csrc/gather_common.cuh.
"""
from typing import NamedTuple

import numpy as np
import torch

from . import _lib as L
from .functional import _require_cuda
from .pretrain_utils import LoadedObs

MAX_SENSORS = 8          # M3L_MAX_SENSORS (csrc/kernels.h)
_DTYPES = {np.dtype(np.uint8): torch.uint8, np.dtype(np.float32): torch.float32}


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _store_dtype(key, dt):
    if isinstance(dt, torch.dtype):
        if dt in (torch.uint8, torch.float32):
            return dt
        raise ValueError(f"observation '{key}': dtype {dt} is not supported (uint8 or float32)")
    try:
        return _DTYPES[np.dtype(dt)]
    except (KeyError, TypeError):
        raise ValueError(f"observation '{key}': dtype {dt} is not supported (uint8 or float32)") from None


def _require_device(who, device, kind, host_class):
    """The device of a device-resident buffer (DeviceRolloutBuffer, m3l_amd.replay.DeviceReplayBuffer): a CPU placement is refused."""
    device = torch.device(device)
    if device.type != "cuda":
        raise L.M3LError(f"{who}(device={str(device)!r}): the {kind} lives in GPU memory and is read by HIP kernels "
                         f"(no CPU fallback); use SB3's {host_class} for a host-side {kind}")
    return device


def _obs_spec(who, obs_shapes, obs_dtypes, image_normalization, tactile_normalization):
    """The observation layout both device-resident buffers accept: keys 'image' (fs, H, W, 3) and / or 'tactile' (fs, 3 * S, h, w), uint8 or
    float32 -> (shapes, torch dtypes, frame_stack); anything else is a ValueError naming `who`."""
    shapes = {k: tuple(int(v) for v in s) for k, s in obs_shapes.items()}
    unknown = set(shapes) - {"image", "tactile"}
    if unknown or not shapes:
        raise ValueError(f"{who}: observation keys {sorted(shapes)} (expected 'image' and / or 'tactile')")
    dtypes = {k: _store_dtype(k, obs_dtypes[k]) for k in shapes}
    fs = set()
    if "image" in shapes:
        s = shapes["image"]
        if len(s) != 4 or s[3] != 3:
            raise ValueError(f"{who}: image shape {s} is not (frame_stack, H, W, 3)")
        fs.add(s[0])
    if "tactile" in shapes:
        s = shapes["tactile"]
        if len(s) != 4:
            raise ValueError(f"{who}: tactile shape {s} is not (frame_stack, 3 * S, h, w)")
        if s[1] % 3 or not 1 <= s[1] // 3 <= MAX_SENSORS:
            raise ValueError(f"{who}: {s[1]} tactile channels per frame is not 3 * S with 1 <= S <= {MAX_SENSORS}")
        fs.add(s[0])
    if len(fs) != 1:
        raise ValueError(f"{who}: image and tactile observations disagree on the frame stack ({sorted(fs)})")
    for name, r in (("image", image_normalization), ("tactile", tactile_normalization)):
        if np.float32(float(r[1]) - float(r[0])) == 0:
            raise ValueError(f"{who}: empty {name} normalisation range {list(r)}")
    return shapes, dtypes, fs.pop()


def _check_obs(who, obs, shapes, n_envs):
    """One vec-env step of observations against the buffer's layout."""
    if set(obs) != set(shapes):
        raise ValueError(f"{who}: observation keys {sorted(obs)} (expected {sorted(shapes)})")
    for k, s in shapes.items():
        if tuple(obs[k].shape) != (n_envs,) + s:
            raise ValueError(f"{who}: observation '{k}' has shape {tuple(obs[k].shape)} (expected {(n_envs,) + s})")


def _check_stores(who, image_store, tactile_store, frames=False):
    """The (T, n_envs, fs, ...) observation stores of a gather -> (T, n_envs, fs, H, W, th, tw, S).  frames: the stores of single frames of
    m3l_amd.replay.gather_load_frames, (T, n_envs, ...) without the fs axis and named *_frames -> (T, n_envs, H, W, th, tw, S)."""
    ref = image_store if image_store is not None else tactile_store
    lead = 2 if frames else 3
    head = tuple(ref.shape[:lead])
    H = W = th = tw = S = 0
    suffix, layout = ("_frames", "(T, n_envs, ...) tensor of 5") if frames else ("_store", "(T, n_envs, fs, ...) tensor of 6")
    for name, t in (("image" + suffix, image_store), ("tactile" + suffix, tactile_store)):
        if t is not None and (t.dim() != lead + 3 or tuple(t.shape[:lead]) != head or not t.is_contiguous()
                              or t.dtype not in (torch.uint8, torch.float32)):
            raise ValueError(f"{who}: {name} must be a contiguous uint8 / float32 {layout} dimensions")
    if image_store is not None:
        H, W, C = image_store.shape[lead:]
        if C != 3:
            raise ValueError(f"{who}: image{suffix} has {C} channels (3)")
    if tactile_store is not None:
        CH, th, tw = tactile_store.shape[lead:]
        if CH % 3 or not 1 <= CH // 3 <= MAX_SENSORS:
            raise ValueError(f"{who}: tactile{suffix} has {CH} channels per frame (3 * S, 1 <= S <= {MAX_SENSORS})")
        S = CH // 3
    return head + (H, W, th, tw, S)


def _loaded_outputs(B, fs, H, W, th, tw, S, device):
    """Uninitialised outputs of a gather of B rows: (image or None, [tactile1..S])."""
    img = torch.empty(B, 3 * fs, H, W, dtype=torch.float32, device=device) if H else None
    return img, [torch.empty(B, 3 * fs, th, tw, dtype=torch.float32, device=device) for _ in range(S)]


def _as_loaded(img_out, tac_outs):
    out = LoadedObs()
    if img_out is not None:
        out["image"] = img_out
    for s, t in enumerate(tac_outs):
        out["tactile" + str(s + 1)] = t
    return out


def gather_load(image_store, tactile_store, idx, image_normalization=(0, 1), tactile_normalization=(-1, 1)):
    """image_store (T, n_envs, fs, H, W, 3) and / or tactile_store (T, n_envs, fs, 3*S, h, w), uint8 or float32 CUDA tensors, and idx (B) int64
    flat indices of the reference's swapped order -> LoadedObs {'image': (B, 3*fs, H, W), 'tactile1..S': (B, 3*fs, h, w)} float32: what
    `vt_load(_flatten_frame_stack(obs[idx]))` gives, in one launch (m3l_rollout_gather_load)."""
    ref = image_store if image_store is not None else tactile_store
    if ref is None:
        raise ValueError("gather_load: neither an image nor a tactile store")
    for name, t in (("image_store", image_store), ("tactile_store", tactile_store), ("idx", idx)):
        if t is not None:
            _require_cuda(t, "gather_load: " + name)
    if idx.dtype != torch.int64 or idx.dim() != 1 or not idx.is_contiguous():
        raise ValueError("gather_load: idx must be a contiguous 1-D int64 tensor")
    T, n_envs, fs, H, W, th, tw, S = _check_stores("gather_load", image_store, tactile_store)
    B = idx.shape[0]
    img_out, tac_outs = _loaded_outputs(B, fs, H, W, th, tw, S, ref.device)
    L.check(L.lib().m3l_rollout_gather_load(
        L.ptr(image_store), int(image_store is not None and image_store.dtype == torch.uint8), H, W, float(image_normalization[0]),
        float(image_normalization[1]), L.ptr(img_out), L.ptr(tactile_store), int(tactile_store is not None and tactile_store.dtype == torch.uint8),
        th, tw, S, float(tactile_normalization[0]), float(tactile_normalization[1]), L.ptr_array(tac_outs), T, n_envs, fs, L.ptr(idx), B,
        _stream()), "m3l_rollout_gather_load")
    return _as_loaded(img_out, tac_outs)


def gather_rows(actions, values, log_probs, advantages, returns, idx):
    """actions (T, n_envs, A) and four (T, n_envs) float32 CUDA tensors, idx (B) int64 -> (B, A) and four (B), in one launch."""
    for t in (actions, values, log_probs, advantages, returns, idx):
        _require_cuda(t, "gather_rows: every argument")
    T, n_envs, A = actions.shape
    B = idx.shape[0]
    if idx.dtype != torch.int64 or idx.dim() != 1 or not idx.is_contiguous():
        raise ValueError("gather_rows: idx must be a contiguous 1-D int64 tensor")
    for t in (actions, values, log_probs, advantages, returns):
        if t.dtype != torch.float32 or not t.is_contiguous() or tuple(t.shape[:2]) != (T, n_envs):
            raise ValueError("gather_rows: contiguous float32 (T, n_envs, ...) tensors expected")
    out = [torch.empty(B, A, dtype=torch.float32, device=actions.device)] + [torch.empty(B, dtype=torch.float32, device=actions.device) for _ in range(4)]
    L.check(L.lib().m3l_rollout_gather_rows(L.ptr(actions), L.ptr(values), L.ptr(log_probs), L.ptr(advantages), L.ptr(returns), T, n_envs, A,
                                            L.ptr(idx), B, *[L.ptr(t) for t in out], _stream()), "m3l_rollout_gather_rows")
    return tuple(out)


def gae(rewards, values, episode_starts, last_values, dones, gamma, gae_lambda):
    """SB3's `compute_returns_and_advantage` on (T, n_envs) float32 CUDA tensors (last_values, dones: (n_envs)) -> (advantages, returns)."""
    T, n_envs = rewards.shape
    for t, shape in ((rewards, (T, n_envs)), (values, (T, n_envs)), (episode_starts, (T, n_envs)), (last_values, (n_envs,)), (dones, (n_envs,))):
        _require_cuda(t, "gae: every argument")
        if t.dtype != torch.float32 or not t.is_contiguous() or tuple(t.shape) != shape:
            raise ValueError(f"gae: contiguous float32 tensors of shape (T, n_envs) / (n_envs) expected, got {tuple(t.shape)} {t.dtype}")
    adv, ret = torch.empty_like(rewards), torch.empty_like(rewards)
    L.check(L.lib().m3l_rollout_gae(L.ptr(rewards), L.ptr(values), L.ptr(episode_starts), L.ptr(last_values), L.ptr(dones), T, n_envs,
                                    float(gamma), float(gae_lambda), L.ptr(adv), L.ptr(ret), _stream()), "m3l_rollout_gae")
    return adv, ret


class RolloutBatch(NamedTuple):
    """One minibatch: SB3's `DictRolloutBufferSamples` with the observations already loaded (`x`; `observations` names the same object)."""
    x: LoadedObs
    actions: torch.Tensor
    old_values: torch.Tensor
    old_log_prob: torch.Tensor
    advantages: torch.Tensor
    returns: torch.Tensor

    @property
    def observations(self):
        return self.x


class DeviceRolloutBuffer:
    """The surface `PPO_MAE` uses on SB3's `DictRolloutBuffer` — reset, add, full, pos, compute_returns_and_advantage, get — over device memory.

    obs_shapes   {'image': (fs, H, W, 3), 'tactile': (fs, 3*S, h, w)}: the per-environment observation shapes of the vec-env, either key optional
    obs_dtypes   {'image': uint8 | float32, 'tactile': ...} (numpy or torch dtypes)
    The stores — 4.8 GB at PPO's defaults with uint8 images — are allocated by the first add(), not by the constructor.
    """

    def __init__(self, buffer_size, n_envs, obs_shapes, obs_dtypes, action_dim, gamma=0.99, gae_lambda=0.95, image_normalization=[0, 1],
                 tactile_normalization=[-1, 1], device="cuda"):
        self.device = _require_device("DeviceRolloutBuffer", device, "rollout", "DictRolloutBuffer")
        self.buffer_size, self.n_envs, self.action_dim = int(buffer_size), int(n_envs), int(action_dim)
        if self.buffer_size < 1 or self.n_envs < 1 or self.action_dim < 1:
            raise ValueError(f"DeviceRolloutBuffer: buffer_size={buffer_size}, n_envs={n_envs}, action_dim={action_dim} must be positive")
        self.obs_shapes, self.obs_dtypes, self.frame_stack = _obs_spec("DeviceRolloutBuffer", obs_shapes, obs_dtypes, image_normalization,
                                                                       tactile_normalization)
        self.gamma, self.gae_lambda = float(gamma), float(gae_lambda)
        self.image_normalization, self.tactile_normalization = list(image_normalization), list(tactile_normalization)
        self.observations = None
        self.reset()

    # ---- filling
    def _allocate(self):
        T, E, dev = self.buffer_size, self.n_envs, self.device
        self.observations = {k: torch.empty((T, E) + s, dtype=self.obs_dtypes[k], device=dev) for k, s in self.obs_shapes.items()}
        self.actions = torch.empty(T, E, self.action_dim, dtype=torch.float32, device=dev)
        for name in ("rewards", "episode_starts", "values", "log_probs", "advantages", "returns"):
            setattr(self, name, torch.empty(T, E, dtype=torch.float32, device=dev))

    def reset(self):
        self.pos, self.full = 0, False

    def add(self, obs, action, reward, episode_start, value, log_prob):
        """One vec-env step into slot `pos`: each observation key with one host-to-device copy, straight into its place; `value` and `log_prob`
        may be device tensors (the policy's outputs) and are stored without a synchronise."""
        if self.full:
            raise ValueError(f"DeviceRolloutBuffer.add: the buffer is full ({self.buffer_size} steps); call reset() first")
        _check_obs("DeviceRolloutBuffer.add", obs, self.obs_shapes, self.n_envs)
        if self.observations is None:
            self._allocate()
        p = self.pos
        for k in self.obs_shapes:
            self.observations[k][p].copy_(torch.as_tensor(obs[k]))
        self.actions[p].copy_(torch.as_tensor(action).reshape(self.n_envs, self.action_dim))
        self.rewards[p].copy_(torch.as_tensor(reward).reshape(self.n_envs))
        self.episode_starts[p].copy_(torch.as_tensor(episode_start).reshape(self.n_envs))
        self.values[p].copy_(torch.as_tensor(value).detach().reshape(self.n_envs))
        self.log_probs[p].copy_(torch.as_tensor(log_prob).detach().reshape(self.n_envs))
        self.pos += 1
        self.full = self.pos == self.buffer_size

    def compute_returns_and_advantage(self, last_values, dones):
        """GAE(lambda) over the stored rewards / values, in one launch: fills `advantages` and `returns`."""
        if not self.full:
            raise ValueError(f"DeviceRolloutBuffer.compute_returns_and_advantage: {self.pos} of {self.buffer_size} steps stored")
        lv = torch.as_tensor(last_values).detach().to(device=self.device, dtype=torch.float32).reshape(self.n_envs).contiguous()
        d = torch.as_tensor(np.asarray(dones, dtype=np.float32) if not isinstance(dones, torch.Tensor) else dones)
        d = d.to(device=self.device, dtype=torch.float32).reshape(self.n_envs).contiguous()
        self.advantages, self.returns = gae(self.rewards, self.values, self.episode_starts, lv, d, self.gamma, self.gae_lambda)

    # ---- sampling
    def _indices(self, indices):
        n = self.buffer_size * self.n_envs
        if indices is None:
            return torch.randperm(n, device=self.device)
        host = torch.as_tensor(indices).detach().cpu()          # injected indices are checked on the host: the kernels cannot report one
        if host.dim() != 1 or host.dtype not in (torch.int64, torch.int32) or host.numel() == 0:
            raise ValueError("DeviceRolloutBuffer.get: indices must be a non-empty 1-D integer sequence")
        if int(host.min()) < 0 or int(host.max()) >= n:
            raise ValueError(f"DeviceRolloutBuffer.get: indices outside [0, {n})")
        return host.to(device=self.device, dtype=torch.int64)

    def get(self, batch_size=None, indices=None):
        """Minibatches in the order of `indices` (flat, the reference's swapped order: env = j // T, t = j % T), or of a permutation drawn with
        torch.randperm on the device.  Like SB3's, the last batch is short when the index count is no multiple of batch_size.  Two launches per
        batch: the observations (gather + flatten + vt_load) and the per-step scalars."""
        if not self.full:
            raise ValueError(f"DeviceRolloutBuffer.get: the buffer is not full ({self.pos} of {self.buffer_size} steps stored)")
        perm = self._indices(indices)
        n = perm.shape[0]
        batch_size = n if batch_size is None else int(batch_size)
        if batch_size < 1:
            raise ValueError(f"DeviceRolloutBuffer.get: batch_size={batch_size}")
        return (self._batch(perm[start:start + batch_size]) for start in range(0, n, batch_size))

    def _batch(self, idx):
        x = gather_load(self.observations.get("image"), self.observations.get("tactile"), idx, self.image_normalization, self.tactile_normalization)
        return RolloutBatch(x, *gather_rows(self.actions, self.values, self.log_probs, self.advantages, self.returns, idx))
