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
replay buffer is m3l_amd.replay.DeviceReplayBuffer, which shares this module's validation — the pad and shift rules of `random_shift` among
it — and csrc/gather_common.cuh.

Two features of the replay buffer's gather carry over, both read-side address changes of the same one gather launch; neither the reference tree
nor SB3 has them: restated in tests/rollout_aug_cases.py, parity unpinned (include/m3l_amd.h "rollout augmentation and frame store").

`random_shift=p` (or `dict(image=p_i, tactile=p_t)`) is the random-shift augmentation of RAD (Laskin et al. 2020), which was introduced on PPO:
the minibatch is augmented at update time and the rollout's stored old_log_prob / values stay as they are.  `shifts` (B, 2, 2) int32 holds one
(dy, dx) per [sample, modality (0 image, 1 tactile)] — a minibatch has one observation dict, so there is no half axis — shared by all frames of
the stack, all channels and all sensors; the kernel clamps every entry to [-p, p].  With x the unaugmented tensor (B, 3 fs, H, W),

    out[b, c, y, x] = x[b, c, clamp(y + dy, 0, H - 1), clamp(x + dx, 0, W - 1)]

bit for bit (m3l_rollout_gather_load_shift / m3l_rollout_gather_load_frames_shift).  `get()` draws every batch's shifts with one torch.randint
per distinct nonzero pad on the device, reads nothing back and keeps the last batch's tensor in `last_shifts`; `get(indices=, shifts=)` injects
an (N, 2, 2) tensor for the whole index list (the parity seam; zeros give the unaugmented batch).  `batch.x` feeds `mae(x)` and the extractor
alike, so both see the augmented observations.

`frame_dedup=True` stores every frame once.  The reference's FrameStack wrapper makes every observation the last fs frames of its episode, so the
stacked store holds each frame fs times (4.8 GB at PPO's defaults with uint8 images; 1.2 GB deduplicated).  `frames[k]` has buffer_size + fs - 1
slots: slot t + fs - 1 holds the newest frame of step t's observation, slots 0 .. fs - 2 the older frames of step 0's stack, uploaded from the
stack that add() receives at pos == 0.  `ages` (T, n_envs) int32 says how many earlier frames of its episode a step's stack reaches, and frame k
of step (t, e) is read from slot t + fs - 1 - min(fs - 1 - k, clamp(ages[t, e], 0, fs - 1)) (m3l_rollout_gather_load_frames).  A rollout is
filled front to back and reset: no wrap, no modulo, and every step stays sampleable.  The ages are kept per environment on the host from
`episode_start`: at pos == 0, 0 at an episode start and else fs - 1 (the prologue holds the real stack, so full reach is exact whatever the
episode's true age); afterwards 0 at an episode start and else min(previous + 1, fs - 1).
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


MAX_SHIFT_PAD = 1 << 15                 # pads of the random shift lie in [0, 2^15)


def _check_pad(who, name, p):
    if isinstance(p, bool) or not isinstance(p, (int, np.integer)) or int(p) < 0:
        raise ValueError(f"{who}: the {name} pad {p!r} must be an integer >= 0")
    if int(p) >= MAX_SHIFT_PAD:
        raise ValueError(f"{who}: the {name} pad {p!r} must be below 2^15 = {MAX_SHIFT_PAD}")
    return int(p)


def _check_shifts(who, shifts, B, device=None, halves=True):
    """shifts int32, contiguous, on the device: (B, 2, 2, 2) [sample, half, modality, (dy, dx)] for the replay buffer's two observation dicts
    (halves), (B, 2, 2) [sample, modality, (dy, dx)] for the rollout's one."""
    shape = (B, 2, 2, 2) if halves else (B, 2, 2)
    if not isinstance(shifts, torch.Tensor) or shifts.dtype != torch.int32 or tuple(shifts.shape) != shape or not shifts.is_contiguous():
        raise ValueError(f"{who}: shifts must be a contiguous int32 tensor of shape {'(B, 2, 2, 2)' if halves else '(B, 2, 2)'} = {shape}: "
                         f"[sample, {'half, ' if halves else ''}modality, (dy, dx)]")
    _require_cuda(shifts, who + ": shifts")
    if device is not None and shifts.device != device:
        raise ValueError(f"{who}: shifts lies on {shifts.device}, the stores on {device}")


def _check_shift_pad(who, shift_pad):
    """The `shift_pad` keyword of the functional gathers -> (image_pad, tactile_pad)."""
    try:
        image_pad, tactile_pad = shift_pad
    except (TypeError, ValueError):
        raise ValueError(f"{who}: shift_pad must be a pair (image_pad, tactile_pad)") from None
    return _check_pad(who, "image", image_pad), _check_pad(who, "tactile", tactile_pad)


def _shift_pads(who, random_shift, obs_shapes):
    """The `random_shift` keyword of both device-resident buffers -> None (off) or (image_pad, tactile_pad) with a nonzero entry; `who` is
    "<class>: random_shift"."""
    if random_shift is None:
        return None
    if isinstance(random_shift, dict):
        unknown = sorted(str(k) for k in random_shift if k not in ("image", "tactile"))
        if unknown:
            raise ValueError(f"{who} has the key(s) {unknown}; it takes 'image' and 'tactile'")
        pads = {k: _check_pad(who, k, random_shift.get(k, 0)) for k in ("image", "tactile")}
    else:
        p = _check_pad(who, "image and tactile", random_shift)
        pads = {k: (p if k in obs_shapes else 0) for k in ("image", "tactile")}      # one integer: every modality the buffer stores
    for k, v in pads.items():
        if v and k not in obs_shapes:
            raise ValueError(f"{who}: a pad of {v} for '{k}', which the buffer does not store (obs_shapes has {sorted(obs_shapes)})")
    return (pads["image"], pads["tactile"]) if any(pads.values()) else None


def _draw_shifts(pads, shape, device):
    """Random shifts of `shape` = (B, [2,] 2, 2) int32 on the device, the last two axes [modality, (dy, dx)]: one torch.randint over [-p, p] per
    distinct nonzero pad (one call when the pads are equal), nothing read back; a modality with pad 0 keeps zeros."""
    pi, pt = pads
    if pi == pt:
        return torch.randint(-pi, pi + 1, shape, dtype=torch.int32, device=device)
    shifts = torch.zeros(shape, dtype=torch.int32, device=device)
    for m, p in ((0, pi), (1, pt)):
        if p:
            shifts[..., m, :] = torch.randint(-p, p + 1, shape[:-2] + (2,), dtype=torch.int32, device=device)
    return shifts


def _gather(who, image, tactile, idx, image_normalization, tactile_normalization, ages=None, frame_stack=None, shifts=None, shift_pad=(0, 0)):
    """What `gather_load` (ages None) and `gather_load_frames` share: the checks, the outputs, the argument list and the entry point."""
    frames = ages is not None or frame_stack is not None
    kind = "frames" if frames else "store"
    ref = image if image is not None else tactile
    if ref is None:
        raise ValueError(f"{who}: neither an image nor a tactile {'frame store' if frames else 'store'}")
    for name, t in ((f"image_{kind}", image), (f"tactile_{kind}", tactile), ("idx", idx)):
        if t is not None:
            _require_cuda(t, f"{who}: {name}")
    if idx.dtype != torch.int64 or idx.dim() != 1 or not idx.is_contiguous():
        raise ValueError(f"{who}: idx must be a contiguous 1-D int64 tensor")
    if frames:
        fs = int(frame_stack)
        if fs < 1:
            raise ValueError(f"{who}: frame_stack={frame_stack}")
        slots, n_envs, H, W, th, tw, S = _check_stores(who, image, tactile, frames=True)
        T = slots - (fs - 1)
        if T < 1:
            raise ValueError(f"{who}: frame stores of {slots} slots hold no step at frame_stack={fs} (T + frame_stack - 1 slots)")
        if not isinstance(ages, torch.Tensor):
            raise ValueError(f"{who}: ages must be a contiguous int32 tensor of shape (T, n_envs) = {(T, n_envs)}")
        _require_cuda(ages, who + ": ages")
        if ages.dtype != torch.int32 or tuple(ages.shape) != (T, n_envs) or not ages.is_contiguous():
            raise ValueError(f"{who}: ages must be a contiguous int32 tensor of shape (T, n_envs) = {(T, n_envs)}")
    else:
        T, n_envs, fs, H, W, th, tw, S = _check_stores(who, image, tactile)
    B = idx.shape[0]
    image_pad, tactile_pad = _check_shift_pad(who, shift_pad)
    if shifts is not None:
        _check_shifts(who, shifts, B, ref.device, halves=False)
    # a pad of a modality that is not stored shifts nothing
    shifted = shifts is not None and bool((image is not None and image_pad) or (tactile is not None and tactile_pad))
    img_out, tac_outs = _loaded_outputs(B, fs, H, W, th, tw, S, ref.device)
    args = (L.ptr(image), int(image is not None and image.dtype == torch.uint8), H, W, float(image_normalization[0]), float(image_normalization[1]),
            L.ptr(img_out), L.ptr(tactile), int(tactile is not None and tactile.dtype == torch.uint8), th, tw, S, float(tactile_normalization[0]),
            float(tactile_normalization[1]), L.ptr_array(tac_outs)) + ((L.ptr(ages),) if frames else ()) + (T, n_envs, fs, L.ptr(idx))
    entry = "m3l_rollout_gather_load" + ("_frames" if frames else "")
    if shifted:         # without a shift the entry points of before run
        entry, args = entry + "_shift", args + (L.ptr(shifts), image_pad, tactile_pad)
    L.check(getattr(L.lib(), entry)(*args, B, _stream()), entry)
    return _as_loaded(img_out, tac_outs)


def gather_load(image_store, tactile_store, idx, image_normalization=(0, 1), tactile_normalization=(-1, 1), shifts=None, shift_pad=(0, 0)):
    """image_store (T, n_envs, fs, H, W, 3) and / or tactile_store (T, n_envs, fs, 3*S, h, w), uint8 or float32 CUDA tensors, and idx (B) int64
    flat indices of the reference's swapped order -> LoadedObs {'image': (B, 3*fs, H, W), 'tactile1..S': (B, 3*fs, h, w)} float32: what
    `vt_load(_flatten_frame_stack(obs[idx]))` gives, in one launch (m3l_rollout_gather_load).
    shifts (B, 2, 2) int32 [sample, modality (0 image, 1 tactile), (dy, dx)] with shift_pad = (image_pad, tactile_pad): the random shift of the
    module's docstring, out[y, x] = in[clamp(y + dy), clamp(x + dx)] with every shift clamped to its modality's pad, in the same one launch
    (m3l_rollout_gather_load_shift).  Without shifts, or with no nonzero pad of a stored modality, m3l_rollout_gather_load runs."""
    return _gather("gather_load", image_store, tactile_store, idx, image_normalization, tactile_normalization, shifts=shifts, shift_pad=shift_pad)


def gather_load_frames(image_frames, tactile_frames, ages, idx, frame_stack, image_normalization=(0, 1), tactile_normalization=(-1, 1), shifts=None,
                       shift_pad=(0, 0)):
    """`gather_load` on the rollout's frame stores: image_frames (T + fs - 1, n_envs, H, W, 3) and / or tactile_frames (T + fs - 1, n_envs, 3*S,
    h, w), uint8 or float32 CUDA tensors — slot t + fs - 1 holds the newest frame of step t's observation, slots 0 .. fs - 2 the older frames of
    step 0's stack — ages (T, n_envs) int32, how many earlier frames of its episode the stack of a step reaches (clamped by the kernel to
    [0, fs - 1]), and idx (B) int64 flat indices -> the LoadedObs `gather_load` returns, in one launch (m3l_rollout_gather_load_frames).  Frame k
    of step (t, e) is read from slot t + fs - 1 - min(fs - 1 - k, age).  shifts, shift_pad: as for `gather_load`
    (m3l_rollout_gather_load_frames_shift)."""
    return _gather("gather_load_frames", image_frames, tactile_frames, idx, image_normalization, tactile_normalization, ages, frame_stack, shifts,
                   shift_pad)


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
    The stores — 4.8 GB at PPO's defaults with uint8 images, `store_bytes()` has the figure — are allocated by the first add(), not by the
    constructor.

    frame_dedup     store every frame once: `frames` {'image': (T + fs - 1, n_envs, H, W, 3), 'tactile': (T + fs - 1, n_envs, 3*S, h, w)} and
                    `ages` (T, n_envs) int32 stand where `observations` stands without it (`observations` is then None).  add() keeps its
                    signature: at pos == 0 it uploads the whole stack into slots 0 .. fs - 1, afterwards only the newest frame of each key into
                    slot pos + fs - 1, and it follows the episodes on the host from `episode_start`, which must live there.  The contract is
                    that of the replay's frame_dedup: the observations are the rolling stacks of the reference's FrameStack wrapper —
                    obs[:, :-1] equal to the previous add()'s obs[:, 1:] within an episode, a constant stack at an episode's first step.  Every
                    step stays sampleable (no deviation from SB3).  reset() keeps the per-environment ages: the next rollout goes on where
                    this one ended.
    check_stacking  with frame_dedup: every add() verifies that contract with torch ops on the device and one read-back — it synchronises: for
                    tests and a first run — and raises ValueError naming the key, the environment and the rule.
    random_shift    the random-shift augmentation of the minibatches (the module's docstring has the rule): None is off — no new array, no new
                    launch, the entry point of before — an integer p pads both modalities by p, dict(image=p_i, tactile=p_t) sets them
                    separately (a missing key: 0); all pads 0 is None.  `get()` draws the shifts on the device, or takes `shifts=`, and keeps
                    the tensor of the last batch in `last_shifts`.  A pad must be an integer in [0, 2^15), and 0 for a modality that is not
                    stored.  The stored scalars (old_log_prob, values, ...) are those of the rollout, as RAD has them.
    """

    def __init__(self, buffer_size, n_envs, obs_shapes, obs_dtypes, action_dim, gamma=0.99, gae_lambda=0.95, image_normalization=[0, 1],
                 tactile_normalization=[-1, 1], device="cuda", frame_dedup=False, check_stacking=False, random_shift=None):
        self.device = _require_device("DeviceRolloutBuffer", device, "rollout", "DictRolloutBuffer")
        self.buffer_size, self.n_envs, self.action_dim = int(buffer_size), int(n_envs), int(action_dim)
        if self.buffer_size < 1 or self.n_envs < 1 or self.action_dim < 1:
            raise ValueError(f"DeviceRolloutBuffer: buffer_size={buffer_size}, n_envs={n_envs}, action_dim={action_dim} must be positive")
        self.obs_shapes, self.obs_dtypes, self.frame_stack = _obs_spec("DeviceRolloutBuffer", obs_shapes, obs_dtypes, image_normalization,
                                                                       tactile_normalization)
        self.gamma, self.gae_lambda = float(gamma), float(gae_lambda)
        self.image_normalization, self.tactile_normalization = list(image_normalization), list(tactile_normalization)
        self.frame_dedup, self.check_stacking = bool(frame_dedup), bool(check_stacking)
        if self.check_stacking and not self.frame_dedup:
            raise ValueError("DeviceRolloutBuffer: check_stacking=True checks the contract of frame_dedup=True and needs it")
        self.random_shift = _shift_pads("DeviceRolloutBuffer: random_shift", random_shift, self.obs_shapes)      # None, or (image_pad, tactile_pad)
        self.last_shifts = None
        self.observations = self.frames = self.ages = None
        # frame_dedup, per environment on the host; reset() keeps them: the age of the last stored step and, for check_stacking, its stack
        self._age = np.zeros(self.n_envs, dtype=np.int32)
        self._last_obs = None
        self.reset()

    # ---- memory
    def store_bytes(self):
        """Bytes of the stores, before or after allocation: {'observations', 'scalars', 'total'}.  With frame_dedup 'observations' is the frame
        stores of buffer_size + frame_stack - 1 slots and 'scalars' counts the 4 bytes per (step, environment) of `ages`."""
        T, fs = self.buffer_size, self.frame_stack
        per_step = lambda shapes: sum(int(np.prod(s)) * torch.empty(0, dtype=self.obs_dtypes[k]).element_size()      # noqa: E731
                                      for k, s in shapes.items()) * self.n_envs
        if self.frame_dedup:
            obs = per_step({k: s[1:] for k, s in self.obs_shapes.items()}) * (T + fs - 1)
        else:
            obs = per_step(self.obs_shapes) * T
        scalars = 4 * T * self.n_envs * (self.action_dim + 6 + int(self.frame_dedup))
        return {"observations": obs, "scalars": scalars, "total": obs + scalars}

    # ---- filling
    def _allocate(self):
        T, E, dev = self.buffer_size, self.n_envs, self.device
        if self.frame_dedup:
            self.frames = {k: torch.empty((T + self.frame_stack - 1, E) + s[1:], dtype=self.obs_dtypes[k], device=dev) for k, s in self.obs_shapes.items()}
            self.ages = torch.empty(T, E, dtype=torch.int32, device=dev)
        else:
            self.observations = {k: torch.empty((T, E) + s, dtype=self.obs_dtypes[k], device=dev) for k, s in self.obs_shapes.items()}
        self.actions = torch.empty(T, E, self.action_dim, dtype=torch.float32, device=dev)
        for name in ("rewards", "episode_starts", "values", "log_probs", "advantages", "returns"):
            setattr(self, name, torch.empty(T, E, dtype=torch.float32, device=dev))

    def reset(self):
        self.pos, self.full = 0, False

    def add(self, obs, action, reward, episode_start, value, log_prob):
        """One vec-env step into slot `pos`: each observation key with one host-to-device copy, straight into its place; `value` and `log_prob`
        may be device tensors (the policy's outputs) and are stored without a synchronise.  With frame_dedup the same full stacked dict is
        taken and only its newest frames are copied (`_add_frames`)."""
        if self.full:
            raise ValueError(f"DeviceRolloutBuffer.add: the buffer is full ({self.buffer_size} steps); call reset() first")
        _check_obs("DeviceRolloutBuffer.add", obs, self.obs_shapes, self.n_envs)
        if self.frame_dedup:
            start = torch.as_tensor(episode_start).reshape(self.n_envs)
            if start.is_cuda:
                raise ValueError("DeviceRolloutBuffer.add: frame_dedup=True follows the episodes on the host and needs `episode_start` there")
        if (self.frames if self.frame_dedup else self.observations) is None:
            self._allocate()
        p = self.pos
        if self.frame_dedup:
            self._add_frames(obs, start.numpy().astype(bool))
        else:
            for k in self.obs_shapes:
                self.observations[k][p].copy_(torch.as_tensor(obs[k]))
        self.actions[p].copy_(torch.as_tensor(action).reshape(self.n_envs, self.action_dim))
        self.rewards[p].copy_(torch.as_tensor(reward).reshape(self.n_envs))
        self.episode_starts[p].copy_(torch.as_tensor(episode_start).reshape(self.n_envs))
        self.values[p].copy_(torch.as_tensor(value).detach().reshape(self.n_envs))
        self.log_probs[p].copy_(torch.as_tensor(log_prob).detach().reshape(self.n_envs))
        self.pos += 1
        self.full = self.pos == self.buffer_size

    _STACKING_RULES = ("all frames of obs are equal at an episode's first step", "obs[:, :-1] equals the previous add()'s obs[:, 1:]")

    def _add_frames(self, obs, start):
        """frame_dedup: at pos == 0 the whole stack into slots 0 .. fs - 1 (the prologue and step 0's newest frame), afterwards the newest frame
        of each key into slot pos + fs - 1; and the step's ages.  At pos == 0 the prologue holds the real stack, so an age of fs - 1 is exact
        whatever the episode's true age."""
        p, fs = self.pos, self.frame_stack
        grown = np.full(self.n_envs, fs - 1, dtype=np.int32) if p == 0 else np.minimum(self._age + 1, fs - 1)
        age = np.where(start, 0, grown).astype(np.int32)
        checked = self._check_stacking(obs, start) if self.check_stacking else None
        for k in self.obs_shapes:
            o = torch.as_tensor(obs[k])
            if p == 0:
                self.frames[k][:fs].copy_(o.transpose(0, 1))
            else:
                self.frames[k][p + fs - 1].copy_(o[:, -1])
        self.ages[p].copy_(torch.from_numpy(age))
        self._age, self._last_obs = age, checked

    def _check_stacking(self, obs, start):
        """The stacking contract of this add() on the device, with one read-back -> obs on the device, for the next add()'s check."""
        first = torch.from_numpy(start).to(self.device)
        rows = lambda x: x.reshape(self.n_envs, -1)      # noqa: E731
        flags, cur = [], {}
        for k in self.obs_shapes:
            o = torch.as_tensor(obs[k]).to(self.device)
            constant = (rows(o[:, 1:]) == rows(o[:, :-1])).all(1) | ~first
            rolls = torch.ones_like(first) if self._last_obs is None else (rows(o[:, :-1]) == rows(self._last_obs[k][:, 1:])).all(1) | first
            flags.append(torch.stack([constant, rolls]))
            cur[k] = o
        ok = torch.stack(flags).cpu().numpy()
        for i, k in enumerate(self.obs_shapes):
            for r, rule in enumerate(self._STACKING_RULES):
                if not ok[i, r].all():
                    e = int(np.flatnonzero(~ok[i, r])[0])
                    raise ValueError(f"DeviceRolloutBuffer.add: check_stacking: observation '{k}' of environment {e} breaks the contract of "
                                     f"frame_dedup=True: {rule} (step {self.pos} of the rollout)")
        return cur

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

    def _check_injected_shifts(self, shifts, indices):
        """`get(shifts=)` checked before anything is launched: it belongs to random_shift and has one entry per index."""
        who = "DeviceRolloutBuffer.get"
        if self.random_shift is None:
            raise ValueError(f"{who}: shifts= belongs to a buffer built with random_shift")
        if indices is None:
            raise ValueError(f"{who}: shifts= needs indices=: it holds one shift per entry of the index list")
        try:
            n = len(indices)
        except TypeError:
            raise ValueError(f"{who}: indices must be a non-empty 1-D integer sequence") from None
        _check_shifts(who, shifts, n, self.device, halves=False)

    def get(self, batch_size=None, indices=None, shifts=None):
        """Minibatches in the order of `indices` (flat, the reference's swapped order: env = j // T, t = j % T), or of a permutation drawn with
        torch.randperm on the device.  Like SB3's, the last batch is short when the index count is no multiple of batch_size.  Two launches per
        batch: the observations (gather + flatten + vt_load) and the per-step scalars.
        random_shift: the observations leave the same gather launch augmented, every batch with shifts of its own from one torch.randint per
        distinct nonzero pad on the device (nothing is read back), or with its slice of the injected int32 tensor `shifts` (N, 2, 2), one
        entry per index (the parity seam; zeros: the unaugmented batch); the tensor of the last batch is kept in `last_shifts`."""
        if shifts is not None:
            self._check_injected_shifts(shifts, indices)
        if not self.full:
            raise ValueError(f"DeviceRolloutBuffer.get: the buffer is not full ({self.pos} of {self.buffer_size} steps stored)")
        perm = self._indices(indices)
        n = perm.shape[0]
        batch_size = n if batch_size is None else int(batch_size)
        if batch_size < 1:
            raise ValueError(f"DeviceRolloutBuffer.get: batch_size={batch_size}")
        # one batch over the whole list takes the injected tensor itself, so that `last_shifts` is that tensor
        cut = lambda start: shifts if batch_size >= n else shifts[start:start + batch_size]      # noqa: E731
        return (self._batch(perm[start:start + batch_size], None if shifts is None else cut(start)) for start in range(0, n, batch_size))

    def _batch(self, idx, shifts=None):
        aug = {}
        if self.random_shift is not None:
            if shifts is None:
                shifts = _draw_shifts(self.random_shift, (idx.shape[0], 2, 2), self.device)
            self.last_shifts = shifts
            aug = dict(shifts=shifts, shift_pad=self.random_shift)
        if self.frame_dedup:
            x = gather_load_frames(self.frames.get("image"), self.frames.get("tactile"), self.ages, idx, self.frame_stack, self.image_normalization,
                                   self.tactile_normalization, **aug)
        else:
            x = gather_load(self.observations.get("image"), self.observations.get("tactile"), idx, self.image_normalization,
                            self.tactile_normalization, **aug)
        return RolloutBatch(x, *gather_rows(self.actions, self.values, self.log_probs, self.advantages, self.returns, idx))
