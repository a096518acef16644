"""The n-step rule of DeviceReplayBuffer(n_steps=, gamma=) restated in numpy / float64 (test_replay_nstep_cpu.py, test_replay_nstep_gpu.py,
test_memory_contract_nstep_gpu.py), over the stores of replay_cases / replay_frame_cases.

SB3's `NStepReplayBuffer` (2.7) is not in the reference tree — the reference pins 2.3.2 — so the rule is restated from include/m3l_amd.h
("n-step returns") and nothing pins the restatement (parity unpinned); the hand-written walks of test_replay_nstep_cpu.py hold it.

Ring of T steps x n_envs, a sampled (t, e), n = n_steps, g = float32(gamma), newest = the step written last:
  walk       k* = the smallest k in [0, n - 1] with dones[(t + k) % T, e] != 0 or (t + k) % T == newest, else n - 1;  last = (t + k*) % T
  rewards    sum_{k <= k*} g^k r~[(t + k) % T, e], r~ the float32 (normalised) reward of replay_cases.normalize_reward_reference, which the
             one-step kernel matches bit for bit; here the powers and the sum are float64, so the only rounding a comparison has to bound is
             that of the kernel's own n float32 products and n - 1 float32 sums: `reward_bound` = 2 n 2^-23 sum_k |g^k r~_k| per sample
  dones      dones[last, e] (1 - timeouts[last, e])
  discounts  g^(k* + 1) in float64; the kernel's repeated float32 multiplication stays within n 2^-23 of it, relatively
  next_observations  the next observation of (last, e);  next_rows = last n_envs + e;  observations, actions, rows: those of (t, e)
`kind` names what ended a walk, the first that applies at k*: 'truncated' (a done with its timeout flag), 'done', 'write_head', 'full'."""
import numpy as np

import replay_cases as PC
import replay_frame_cases as FC

KINDS = ("done", "truncated", "write_head", "full")
EPS = 2.0 ** -23


def walk(dones, timeouts, t, e, T, n, newest):
    """One walk on dones / timeouts (T, n_envs) (timeouts may be None: then no walk is 'truncated') -> (k*, last, kind, wrapped)."""
    for k in range(n):
        s = (t + k) % T
        if dones[s, e] != 0:
            truncated = timeouts is not None and timeouts[s, e] != 0
            return k, s, "truncated" if truncated else "done", t + k >= T
        if s == newest:
            return k, s, "write_head", t + k >= T
    return n - 1, (t + n - 1) % T, "full", t + n - 1 >= T


def nstep_reference(scalars, t, e, T, n, gamma, newest, reward_norm=None):
    """scalars as replay_cases.sample_reference takes them, steps t and environments e (B) -> dict(k_star, last (B) int64, kind [B], wrapped (B)
    bool, rewards, dones, discounts, reward_bound (B, 1) float64 (dones exact in float32), actions (B, A), rows, next_rows (B) int64)."""
    t, e = np.asarray(t, dtype=np.int64), np.asarray(e, dtype=np.int64)
    n_envs = scalars["dones"].shape[1]
    r32 = scalars["rewards"].astype(np.float32)
    if reward_norm is not None:
        r32 = PC.normalize_reward_reference(r32, *reward_norm)
    assert r32.dtype == np.float32
    g = np.float64(np.float32(gamma))
    out = dict(k_star=[], last=[], kind=[], wrapped=[], rewards=[], dones=[], discounts=[], reward_bound=[])
    for tt, ee in zip(t.tolist(), e.tolist()):
        k_star, last, kind, wrapped = walk(scalars["dones"], scalars.get("timeouts"), tt, ee, T, n, newest)
        terms = [g ** k * np.float64(r32[(tt + k) % T, ee]) for k in range(k_star + 1)]
        done = np.float32(scalars["dones"][last, ee])
        if scalars.get("timeouts") is not None:
            done = done * (np.float32(1) - np.float32(scalars["timeouts"][last, ee]))
        for name, v in (("k_star", k_star), ("last", last), ("kind", kind), ("wrapped", wrapped), ("rewards", sum(terms)), ("dones", done),
                        ("discounts", g ** (k_star + 1)), ("reward_bound", 2 * n * EPS * sum(abs(x) for x in terms))):
            out[name].append(v)
    col = lambda v, dt: np.asarray(v, dtype=dt).reshape(-1, 1)      # noqa: E731
    last = np.asarray(out["last"], dtype=np.int64)
    return dict(k_star=np.asarray(out["k_star"], dtype=np.int64), last=last, kind=out["kind"], wrapped=np.asarray(out["wrapped"], dtype=bool),
                rewards=col(out["rewards"], np.float64), dones=col(out["dones"], np.float32), discounts=col(out["discounts"], np.float64),
                reward_bound=col(out["reward_bound"], np.float64), actions=scalars["actions"][t, e], rows=t * n_envs + e,
                next_rows=last * n_envs + e)


def sample_reference(stores, next_stores, scalars, t, e, T, n, gamma, newest, reward_norm=None, image_normalization=(0, 1),
                     tactile_normalization=(-1, 1)):
    """`nstep_reference` plus observations of (t, e) and next_observations of (last, e) from the two-store numpy stacks, through
    replay_cases.sample_reference (the reference's flatten and vt_load)."""
    assert next_stores is not None, "n-step returns need the two-store mode"
    out = nstep_reference(scalars, t, e, T, n, gamma, newest, reward_norm)
    first = PC.sample_reference(stores, next_stores, scalars, t, e, T, None, image_normalization, tactile_normalization)
    final = PC.sample_reference(stores, next_stores, scalars, out["last"], e, T, None, image_normalization, tactile_normalization)
    out.update(observations=first["observations"], next_observations=final["next_observations"])
    return out


# ---- the stream of the GPU tests: T = 7 steps of 2 environments, checkpoints after 5, 7 and 17 adds, n_steps 1, 2, 3 and 5
T, E, A = 7, 2, 3
CHECKPOINTS = (5, 7, 17)          # not full (newest = 4); just full (pos = 0, newest = 6); wrapped more than twice (pos = 3, newest = 2)
N_STEPS = (1, 2, 3, 5)


def episode_lengths(fs, env):
    """Episode lengths, cycled, chosen for the coverage condition (test_replay_nstep_cpu.py checks it): replay_frame_cases.episode_lengths ends
    an episode every few steps, which leaves no room for a full walk of 5.  Environment 0 starts with an episode of 7 steps (steps 0..5 of the
    first two checkpoints carry no done: full walks of every n) and environment 1 has one that spans the ring end at the third checkpoint;
    both also keep episodes shorter than the frame stack.  In make_stream an episode whose (number + env) is even ends in a truncation."""
    return [[7, 2, 1, 6, 3], [2, 1, 3, 9, 4]][env]


def make_stream(fs, image_hw, tactile_hw, S, image_dtype, tactile_dtype, seed, n_adds=max(CHECKPOINTS)):
    return FC.make_stream(n_adds, E, fs, image_hw, tactile_hw, S, image_dtype, tactile_dtype, A, seed, lengths=episode_lengths)


def valid_pairs(model):
    """Every valid (t, e) of a RingModel / FrameRingModel as two arrays, steps in the model's order."""
    valid = model.valid_steps()
    return np.repeat(valid, E), np.tile(np.arange(E), len(valid))


def coverage(stream, n, fs=None, timeouts=True):
    """Kinds of walk end and the number of walks that wrap the ring end, over every valid (t, e) of every checkpoint of the stream.  fs None:
    the stacked buffer's valid steps; else those of the frame-deduplicated buffer with that frame stack."""
    kinds, wraps = set(), 0
    for c in CHECKPOINTS:
        stacked, frames = FC.fill_models(c, T, fs or 1, False, stream)
        model = stacked if fs is None else frames
        _, _, scalars = FC.stacked_stores(stacked, stream)
        if not timeouts:
            scalars["timeouts"] = None
        t, e = valid_pairs(model)
        ref = nstep_reference(scalars, t, e, T, n, 0.99, (model.pos - 1) % T)
        kinds |= set(ref["kind"])
        wraps += int(ref["wrapped"].sum())
    return kinds, wraps


class RewardNorm:
    """What DeviceReplayBuffer.sample(env=...) reads of a VecNormalize: norm_reward, ret_rms.var, epsilon, clip_reward."""
    class _Rms:
        def __init__(self, var):
            self.var = var

    def __init__(self, var=2.25, epsilon=1e-8, clip_reward=1.5):
        self.norm_obs, self.norm_reward = False, True
        self.ret_rms, self.epsilon, self.clip_reward = self._Rms(var), epsilon, clip_reward

    def triple(self):
        return self.ret_rms.var, self.epsilon, self.clip_reward
