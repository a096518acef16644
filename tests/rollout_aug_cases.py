"""The two read-side features of DeviceRolloutBuffer's gather restated in numpy — the frame store of `frame_dedup=True` and the random shift of
`random_shift=` — and the small rollout streams their tests use (test_rollout_aug_cpu.py, test_rollout_aug_gpu.py,
test_memory_contract_rollout_aug_gpu.py).

Neither the reference tree nor SB3 has either feature: the rules are restated from include/m3l_amd.h ("rollout augmentation and frame store")
and nothing pins the restatement (parity unpinned).  Nothing here has a tolerance: every comparison is bit-equality against integer indexing.

  Shift.  shifts (B, 2, 2) int32: [sample, modality (0 image, 1 tactile), (dy, dx)], every entry clamped to [-pad, pad] of its modality; the
  augmented tensor is shift_cases.random_shift_reference of the unaugmented tensor of the same indices (`shifted_reference`).

  Frame store.  frames (T + fs - 1, n_envs, ...) and ages (T, n_envs): slot t + fs - 1 holds the newest frame of step t's observation, slots
  0 .. fs - 2 the older frames of step 0's stack.  Frame k of step (t, e) is read from slot
      t + fs - 1 - min(fs - 1 - k, clamp(ages[t, e], 0, fs - 1))                                              (`frame_slot`)
  The ages follow `episode_start` per environment: at the rollout's first step 0 at an episode start, else fs - 1 (the prologue holds the real
  stack); afterwards 0 at an episode start, else min(previous + 1, fs - 1)                                       (`next_ages`)

The streams are shift_cases.make_stream's FrameStack-wrapped environments cut into two consecutive rollouts of T steps with a reset() between;
episode_start[k] is True for k = 0 and dones[k - 1] afterwards.  T = 5 and T = 7: the second rollouts then begin at an episode start, in the
middle of an episode younger than the stack, and in the middle of one at least as old (`coverage_missing`)."""
import numpy as np

import shift_cases as SH

E, A = SH.E, SH.A
ROLLOUT_T = (5, 7)                     # steps of one rollout; a stream is two of them
CONFIGS = SH.CONFIGS                   # the 16-byte and element forms of both modalities, uint8 / float32, pad >= W


def frame_slot(t, k, fs, age):
    """Slot of frame k (0 the oldest, fs - 1 the newest) of step t for a stack that reaches `age` earlier frames; any integer age."""
    reach = min(max(int(age), 0), fs - 1)
    return t + fs - 1 - min(fs - 1 - k, reach)


def next_ages(prev, episode_start, fs, first_step):
    """Ages (n_envs) of one add(): prev the ages of the step before (ignored at the rollout's first step)."""
    grown = np.full(len(episode_start), fs - 1) if first_step else np.minimum(np.asarray(prev) + 1, fs - 1)
    return np.where(np.asarray(episode_start, dtype=bool), 0, grown).astype(np.int32)


def frame_store_reference(obs, episode_start, fs):
    """One rollout's stacked observations obs (T, n_envs, fs, ...) and episode_start (T, n_envs) -> frames (T + fs - 1, n_envs, ...), ages
    (T, n_envs): what add() stores, step by step."""
    T, n_envs = obs.shape[:2]
    frames = np.zeros((T + fs - 1, n_envs) + obs.shape[3:], dtype=obs.dtype)
    ages = np.zeros((T, n_envs), dtype=np.int32)
    for t in range(T):
        if t == 0:
            frames[:fs] = obs[0].swapaxes(0, 1)
        else:
            frames[t + fs - 1] = obs[t, :, -1]
        ages[t] = next_ages(ages[t - 1] if t else None, episode_start[t], fs, t == 0)
    return frames, ages


def stacked_from_frames(frames, ages, fs):
    """The stacked store (T, n_envs, fs, ...) that the slot rule reads out of a frame store."""
    T, n_envs = ages.shape
    out = np.zeros((T, n_envs, fs) + frames.shape[2:], dtype=frames.dtype)
    for t in range(T):
        for e in range(n_envs):
            for k in range(fs):
                out[t, e, k] = frames[frame_slot(t, k, fs, ages[t, e]), e]
    return out


def shifted_reference(x, shifts, pads):
    """x {'image': (B, 3 fs, H, W), 'tactile1..S': (B, 3 fs, h, w)} of numpy arrays through shifts (B, 2, 2) and pads (image_pad, tactile_pad):
    the image takes modality 0, every sensor modality 1."""
    shifts = np.asarray(shifts)
    return {k: SH.random_shift_reference(v, shifts[:, 0 if k == "image" else 1], pads[0 if k == "image" else 1]) for k, v in x.items()}


def injected_shifts(pads):
    """(N, 2, 2) int32: every shift of each modality's range, out-of-range entries and the ends of int32 (half 0 of the replay's list)."""
    return np.ascontiguousarray(SH.injected_shifts(pads)[:, 0])


def make_rollouts(name, T, seed):
    """Config `name` -> dict(fs, obs {'image': (2 T, E, fs, H, W, 3), 'tactile': (2 T, E, fs, 3 S, h, w)}, episode_start (2 T, E) bool,
    true_age (2 T, E): steps since the episode began, actions, rewards, values, log_probs (2 T, E[, A]) float32, last_values, dones (2, E)).
    Rollout r is steps [r T, (r + 1) T)."""
    fs, image_hw, tactile_hw, S, dtypes, _ = CONFIGS[name]
    st = SH.make_stream(fs, image_hw, tactile_hw, S, dtypes[0], dtypes[1], seed=seed, n_adds=2 * T)
    start = np.ones((2 * T, E), dtype=bool)
    start[1:] = st["dones"][:-1]
    true_age = np.zeros((2 * T, E), dtype=np.int64)
    for k in range(1, 2 * T):
        true_age[k] = np.where(start[k], 0, true_age[k - 1] + 1)
    g = np.random.default_rng(1000 + seed)
    f = lambda *s: g.standard_normal(s).astype(np.float32)      # noqa: E731
    return dict(fs=fs, T=T, obs=st["obs"], episode_start=start, true_age=true_age, actions=st["actions"], rewards=st["rewards"],
                values=f(2 * T, E), log_probs=f(2 * T, E), last_values=f(2, E), dones=np.stack([st["dones"][T - 1], st["dones"][2 * T - 1]]))


def rollout_slice(ro, r):
    T = ro["T"]
    return slice(r * T, (r + 1) * T)


def coverage_missing(fs=3):
    """What the starts of the second rollouts (stream step T, T in ROLLOUT_T) of a frame stack of fs do not cover -> list of what is missing."""
    name = next(n for n in sorted(CONFIGS) if CONFIGS[n][0] == fs)
    seen = set()
    for T in ROLLOUT_T:
        ro = make_rollouts(name, T, seed=0)
        for e in range(E):
            if ro["episode_start"][T, e]:
                seen.add("an episode start")
            elif ro["true_age"][T, e] < fs - 1:
                seen.add("mid-episode with age < fs - 1")
            else:
                seen.add("mid-episode with true age >= fs - 1")
    return sorted({"an episode start", "mid-episode with age < fs - 1", "mid-episode with true age >= fs - 1"} - seen)
