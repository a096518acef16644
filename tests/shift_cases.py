"""The random-shift augmentation of DeviceReplayBuffer(random_shift=) restated in numpy (test_replay_shift_cpu.py, test_replay_shift_gpu.py,
test_memory_contract_shift_gpu.py), and the small streams and shift lists those tests use.

Neither the reference tree nor SB3 has this augmentation (DrQ, Kostrikov et al. 2021; RAD, Laskin et al. 2020): the rule is restated from
include/m3l_amd.h ("random-shift augmentation") and nothing pins the restatement (parity unpinned); test_replay_shift_cpu.py holds it against
torch's replicate padding and an example written out by hand.

  shifts (B, 2, 2, 2) int32: [sample, half (0 observations, 1 next observations), modality (0 image, 1 tactile), (dy, dx)], every entry clamped
  to [-pad, pad] of its modality; with x the unaugmented tensor of a half, (B, C, H, W):
      out[b, c, y, x] = x[b, c, clamp(y + dy, 0, H - 1), clamp(x + dx, 0, W - 1)]
An augmented batch is this indexing applied to the unaugmented batch of the same rows, bit for bit: nothing here has a tolerance."""
from collections import deque

import numpy as np

INT32_MIN, INT32_MAX = -2 ** 31, 2 ** 31 - 1
OUT_OF_RANGE = ((1000, -1000), (-1000, 1000), (INT32_MAX, INT32_MIN), (INT32_MIN, INT32_MAX))


def clamp_shift(shifts, pad):
    """Entries of any integer type -> int64 entries in [-pad, pad]."""
    return np.clip(np.asarray(shifts, dtype=np.int64), -int(pad), int(pad))


def random_shift_reference(x, shifts_b, pad):
    """x (B, C, H, W), shifts_b (B, 2) integers (dy, dx), pad >= 0 -> out (B, C, H, W) of x's dtype, by integer indexing alone."""
    x = np.asarray(x)
    B, C, H, W = x.shape
    s = clamp_shift(shifts_b, pad).reshape(B, 2)
    ys = np.clip(np.arange(H, dtype=np.int64)[None, :] + s[:, 0:1], 0, H - 1)          # (B, H)
    xs = np.clip(np.arange(W, dtype=np.int64)[None, :] + s[:, 1:2], 0, W - 1)          # (B, W)
    return x[np.arange(B)[:, None, None, None], np.arange(C)[None, :, None, None], ys[:, None, :, None], xs[:, None, None, :]]


def shifted_obs_reference(obs, shifts, half, pads):
    """One half of a batch, {'image': (B, 3 fs, H, W), 'tactile1..S': (B, 3 fs, h, w)} of numpy arrays, through shifts (B, 2, 2, 2) and pads
    (image_pad, tactile_pad): the image takes modality 0, every sensor modality 1."""
    shifts = np.asarray(shifts)
    return {k: random_shift_reference(v, shifts[:, half, 0 if k == "image" else 1], pads[0 if k == "image" else 1]) for k, v in obs.items()}


# ---- the injected shifts of the GPU tests
def shift_list(pad):
    """Every (dy, dx) of [-pad, pad]^2 — the four corners, (0, 0), every dx that is not a multiple of 4, and with pad >= W - 1 the shifts
    that move a whole row out of the frame — then one out-of-range entry per sign and the ends of int32."""
    r = range(-pad, pad + 1)
    return [(dy, dx) for dy in r for dx in r] + list(OUT_OF_RANGE)


def injected_shifts(pads, B=None):
    """shifts (B, 2, 2, 2) int32 for pads (image_pad, tactile_pad): half 0 of sample b takes entry b of its modality's `shift_list`, half 1
    another entry (a stride coprime to the list's length), so the two halves of a sample differ.  B defaults to the longer list's length."""
    lists = [shift_list(p) for p in pads]
    B = max(len(x) for x in lists) if B is None else B
    out = np.zeros((B, 2, 2, 2), dtype=np.int64)
    for m, lst in enumerate(lists):
        n = len(lst)
        stride = next(s for s in (7, 11, 13, 17) if np.gcd(s, n) == 1)
        for b in range(B):
            out[b, 0, m] = lst[b % n]
            out[b, 1, m] = lst[(b * stride + 3) % n]
    return out.astype(np.int32)


def covers(shifts, modality, pad, W):
    """The coverage condition of an injected shift tensor for one modality with pad > 0 and frame width W -> the list of what is missing."""
    s = np.asarray(shifts, dtype=np.int64)[:, :, modality].reshape(-1, 2)
    have = {tuple(v) for v in s.tolist()}
    missing = [f"corner {c}" for c in ((pad, pad), (pad, -pad), (-pad, pad), (-pad, -pad)) if c not in have]
    if (0, 0) not in have:
        missing.append("(0, 0)")
    in_range = s[(np.abs(s) <= pad).all(1)]
    if not (in_range[:, 1] % 4 != 0).any():
        missing.append("a dx that is no multiple of 4")
    if not (np.abs(s[:, 1]) >= W - 1).any():
        missing.append("|dx| >= W - 1")
    if pad >= W - 1 and not (np.abs(in_range[:, 1]) >= W - 1).any():
        missing.append("|dx| >= W - 1 within the pad")
    for sign, name in ((1, "above"), (-1, "below")):
        if not ((sign * s) > pad).any():
            missing.append(f"an entry {name} the range")
    if not ((s == INT32_MIN).any() and (s == INT32_MAX).any()):
        missing.append("INT32_MIN and INT32_MAX")
    return missing


# ---- the streams and stores: ramps with strides coprime to 251, so that neighbouring pixels, rows, channels, frames, sensors, environments and
# steps all differ and a pixel taken from the wrong place cannot compare equal
T, E, A = 7, 2, 3
N_ADDS = 10                         # the ring has wrapped: pos = 3

# name -> frame stack, image (H, W), tactile (h, w), sensors, (image, tactile) dtypes, pads (image, tactile)
CONFIGS = {
    "u8_8x12_f32_4x8_S2_fs2_pads32": (2, (8, 12), (4, 8), 2, (np.uint8, np.float32), (3, 2)),        # both 16-byte forms; H != W
    "f32_5x6_u8_3x5_S1_fs3_pads32": (3, (5, 6), (3, 5), 1, (np.float32, np.uint8), (3, 2)),          # both element forms
    "f32_4x4_u8_4x8_S2_fs3_pads40": (3, (4, 4), (4, 8), 2, (np.float32, np.uint8), (4, 0)),          # every lane an edge lane; pad >= W
    "u8_4x4_f32_3x5_S1_fs2_pads40": (2, (4, 4), (3, 5), 1, (np.uint8, np.float32), (4, 0)),
    "f32_8x12_u8_4x8_S2_fs2_pads32": (2, (8, 12), (4, 8), 2, (np.float32, np.uint8), (3, 2)),
    "u8_5x6_f32_4x8_S2_fs3_pads32": (3, (5, 6), (4, 8), 2, (np.uint8, np.float32), (3, 2)),
}


def ramp_frame(shape, dtype, kind, env, number):
    """Frame `number` of environment `env`: (7 i + 37 number + 101 env + 13 [tactile]) mod 251 over the flat index i — 7, 37 and 101 are coprime
    to 251, and so is 7 times every row and plane length used here — as it is for uint8, and for float32 moved to non-integers: (v + 0.37) / 251
    in [0, 1) for an image, 2 (v + 0.37) / 251 - 1 in [-1, 1) for a tactile frame."""
    i = np.arange(int(np.prod(shape)), dtype=np.int64)
    v = (7 * i + 37 * number + 101 * env + (13 if kind == "tactile" else 0)) % 251
    if np.dtype(dtype) == np.uint8:
        return v.astype(np.uint8).reshape(shape)
    f = (v.astype(np.float64) + 0.37) / 251.0
    return (f if kind == "image" else 2 * f - 1).astype(np.float32).reshape(shape)


def episode_lengths(fs, env):
    """Episode lengths, cycled: shorter than the stack, one step, longer than the stack; the environments end theirs at different steps."""
    return [[fs + 2, 1, 2], [2, fs + 1, 1]][env]


def make_stream(fs, image_hw, tactile_hw, S, image_dtype, tactile_dtype, seed, n_adds=N_ADDS):
    """n_adds consecutive add() calls of E FrameStack-wrapped environments with auto-reset, as the frame-deduplicated store's contract wants
    them (rolling stacks, a constant stack at an episode's first step): dict(obs, next_obs {'image': (n_adds, E, fs, H, W, 3), 'tactile':
    (n_adds, E, fs, 3 S, h, w)}, actions (n_adds, E, A), rewards, dones (n_adds, E), infos [n_adds][E]).  Every second episode end is a
    truncation."""
    spec = {"image": (tuple(image_hw) + (3,), image_dtype), "tactile": ((3 * S,) + tuple(tactile_hw), tactile_dtype)}
    rng = np.random.default_rng(seed)
    count, left, ends = [0] * E, [0] * E, [0] * E
    stacks = [{k: deque([], maxlen=fs) for k in spec} for _ in range(E)]
    episode = [0] * E

    def new_frames(e):
        count[e] += 1
        return {k: ramp_frame(shape, dt, k, e, count[e] - 1) for k, (shape, dt) in spec.items()}

    def reset(e):
        f = new_frames(e)
        for k in spec:
            for _ in range(fs):
                stacks[e][k].append(f[k])
        lengths = episode_lengths(fs, e)
        left[e] = lengths[episode[e] % len(lengths)]
        episode[e] += 1

    for e in range(E):
        reset(e)
    obs = {k: [] for k in spec}
    nxt = {k: [] for k in spec}
    dones, infos = np.zeros((n_adds, E), dtype=bool), []
    for step in range(n_adds):
        row_obs, row_next, info = {k: [] for k in spec}, {k: [] for k in spec}, []
        for e in range(E):
            for k in spec:
                row_obs[k].append(np.stack(stacks[e][k]))
            f = new_frames(e)
            for k in spec:
                stacks[e][k].append(f[k])
                row_next[k].append(np.stack(stacks[e][k]))
            left[e] -= 1
            done = left[e] == 0
            dones[step, e] = done
            truncated = False
            if done:
                ends[e] += 1
                truncated = ends[e] % 2 == 0
                reset(e)
            info.append({"TimeLimit.truncated": truncated})
        for k in spec:
            obs[k].append(np.stack(row_obs[k]))
            nxt[k].append(np.stack(row_next[k]))
        infos.append(info)
    return dict(obs={k: np.stack(v) for k, v in obs.items()}, next_obs={k: np.stack(v) for k, v in nxt.items()},
                actions=(rng.random((n_adds, E, A)) * 2 - 1).astype(np.float32), rewards=(rng.random((n_adds, E)) * 3 - 1.5).astype(np.float32),
                dones=dones, infos=infos)
