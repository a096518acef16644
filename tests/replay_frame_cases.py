"""Restatements and inputs for the tests of the frame-deduplicated replay store (test_replay_frames_cpu.py, test_replay_frames_gpu.py).

gymnasium and stable-baselines3 are not in the reference tree's reach here, so three things are restated from the reference's code and SB3's
documented behaviour, and nothing pins the restatements (parity unpinned); the hand-computed cases of test_replay_frames_cpu.py hold them:

`FrameStack`      the reference's wrapper, utils/frame_stack.py:76-105: step() appends the new frame to a deque of fs, reset() fills the deque
                  with the reset frame, an observation is the stacked deque
`make_stream`     SB3's DummyVecEnv over such environments — when an episode ends the environment is reset at once, the returned observation is
                  the new episode's and the last one of the old episode goes to info['terminal_observation'], with info['TimeLimit.truncated']
                  for a truncation — and `OffPolicyAlgorithm._store_transition`, which puts the terminal observation back as next_obs before
                  `replay_buffer.add(last_obs, next_obs, action, reward, done, infos)`
`FrameRingModel`  tests/replay_cases.py's RingModel with the two rules of the deduplicated store: which frames the stack of a step is made of
                  (observation frame j of step t with age a lies in slot (t - min(fs - 1 - j, a)) mod T) and which steps of a full ring still
                  have their history (not the fs - 1 oldest)

The yardstick of the GPU tests is the stacked DeviceReplayBuffer fed with the same stream, which golden/rollout_feed.npz and
replay_cases.sample_reference pin.
"""
from collections import deque

import numpy as np

import replay_cases as PC
import rollout_cases as RC


class FrameStack:
    """utils/frame_stack.py:76-105 without the gym plumbing: one deque of num_stack frames per observation key."""

    def __init__(self, keys, num_stack):
        self.num_stack = num_stack
        self.frames = {k: deque([], maxlen=num_stack) for k in keys}

    def observation(self):
        for k in self.frames:
            assert len(self.frames[k]) == self.num_stack
        return {k: np.stack(self.frames[k], axis=0) for k in self.frames}

    def step(self, observation):
        for k in self.frames:
            self.frames[k].append(observation[k])
        return self.observation()

    def reset(self, observation):
        for k in self.frames:
            for _ in range(self.num_stack):
                self.frames[k].append(observation[k])
        return self.observation()


def episode_lengths(fs, env):
    """Episode lengths of environment `env`, cycled: 1 (two consecutive steps whose stacks are constant), 2 and fs - 1 (shorter than the stack)
    and fs + 2 + env (longer); every environment starts elsewhere in the list, so the episodes end at different steps."""
    base = [1, 2, fs + 2 + env, max(fs - 1, 1)]
    return base[(2 * env) % 4:] + base[:(2 * env) % 4]


def make_frame(shape, dtype, kind, env, number, rng):
    """One frame of seeded noise whose first two elements encode (env, number of the frame in that environment): no two frames of a stream
    are equal, so a wrong source frame cannot pass for the right one.  uint8 frames cover 0..255, float images [0, 1), float tactile [-1, 1)."""
    assert number < 256
    if np.dtype(dtype) == np.uint8:
        f = rng.integers(0, 256, shape, dtype=np.uint8)
        f.reshape(-1)[:2] = (env, number)
    else:
        f = rng.random(shape, dtype=np.float32)
        if kind == "tactile":
            f = (2 * f - 1).astype(np.float32)
        f.reshape(-1)[:2] = (env / 8, number / 256)          # exact in float32
    return f


def make_stream(n_adds, n_envs, fs, image_hw, tactile_hw, S, image_dtype, tactile_dtype, A, seed, lengths=episode_lengths):
    """n_adds consecutive `add()` calls of a SAC run on n_envs FrameStack-wrapped environments with auto-reset ->
    dict(obs, next_obs: {'image': (n_adds, n_envs, fs, H, W, 3), 'tactile': (n_adds, n_envs, fs, 3 S, h, w)} (a key is left out when its
    size is None), actions (n_adds, n_envs, A), rewards (n_adds, n_envs), dones, timeouts (n_adds, n_envs) bool, infos [n_adds][n_envs],
    ages (n_adds, n_envs): min(steps since the episode's reset, fs - 1), taken from the episode counter itself).
    Episodes with an even (episode number + env) end in a truncation, the others in a termination."""
    rng = np.random.default_rng(seed)
    spec = {}
    if image_hw is not None:
        spec["image"] = (tuple(image_hw) + (3,), image_dtype)
    if tactile_hw is not None:
        spec["tactile"] = ((3 * S,) + tuple(tactile_hw), tactile_dtype)
    count = [0] * n_envs

    def new_frames(e):
        count[e] += 1
        return {k: make_frame(shape, dt, k, e, count[e] - 1, rng) for k, (shape, dt) in spec.items()}

    envs = [FrameStack(spec, fs) for _ in range(n_envs)]
    current = [envs[e].reset(new_frames(e)) for e in range(n_envs)]
    in_episode, episode = [0] * n_envs, [0] * n_envs
    out = dict(obs={k: [] for k in spec}, next_obs={k: [] for k in spec}, dones=[], timeouts=[], ages=[], infos=[])
    for _ in range(n_adds):
        obs, nxt, dones, timeouts, ages, infos = [], [], [], [], [], []
        for e in range(n_envs):
            obs.append(current[e])
            ages.append(min(in_episode[e], fs - 1))
            stepped = envs[e].step(new_frames(e))
            in_episode[e] += 1
            plan = lengths(fs, e)
            done = in_episode[e] == plan[episode[e] % len(plan)]
            truncated = done and (episode[e] + e) % 2 == 0
            nxt.append(stepped)                                # the terminal observation when the episode ended (_store_transition)
            if done:
                infos.append({"terminal_observation": stepped, "TimeLimit.truncated": truncated})
                current[e] = envs[e].reset(new_frames(e))
                in_episode[e], episode[e] = 0, episode[e] + 1
            else:
                infos.append({})
                current[e] = stepped
            dones.append(done)
            timeouts.append(truncated)
        for k in spec:
            out["obs"][k].append(np.stack([o[k] for o in obs]))
            out["next_obs"][k].append(np.stack([o[k] for o in nxt]))
        out["dones"].append(dones)
        out["timeouts"].append(timeouts)
        out["ages"].append(ages)
        out["infos"].append(infos)
    for name in ("obs", "next_obs"):
        out[name] = {k: np.stack(v) for k, v in out[name].items()}
    out["dones"], out["timeouts"] = np.array(out["dones"], bool), np.array(out["timeouts"], bool)
    out["ages"] = np.array(out["ages"], np.int32)
    out["actions"] = rng.standard_normal((n_adds, n_envs, A)).astype(np.float32)
    out["rewards"] = (3 * rng.standard_normal((n_adds, n_envs))).astype(np.float32)
    return out


class FrameRingModel(PC.RingModel):
    """RingModel for the deduplicated store: a tag ('obs' | 'next', k) in `obs[slot]` / `next_obs[slot]` now names the newest frame of that
    observation of the k-th add, and `ages[slot]` holds that add's ages per environment."""

    def __init__(self, T, fs, single_store=False):
        super().__init__(T, single_store)
        self.fs = fs
        self.ages = [None] * T

    def add(self, ages):
        p = self.pos
        super().add()
        self.ages[p] = [int(a) for a in ages]

    def valid_steps(self):
        """Before the ring is full, every stored step.  Full: the T - (fs - 1) steps from pos + fs - 1 with two stores, the T - fs steps from
        pos + fs with one (slot pos holds the newest next frame)."""
        skip = self.fs - 1 + int(self.single_store)
        if self.full and skip:
            return [(self.pos + skip + u) % self.T for u in range(self.T - skip)]
        return list(range(self.size()))

    def obs_frames(self, t, e):
        """Tags of the fs frames of step t's observation, oldest first."""
        a = self.ages[t][e]
        return [self.obs[(t - min(self.fs - 1 - j, a)) % self.T] for j in range(self.fs)]

    def next_frames(self, t, e):
        return self.obs_frames(t, e)[1:] + [self.next_of(t)]


def fill_models(n_adds, T, fs, single_store, stream):
    """The pure-Python models after the first n_adds adds of a stream: (RingModel of the stacked buffer, FrameRingModel)."""
    stacked, frames = PC.RingModel(T, single_store), FrameRingModel(T, fs, single_store)
    for k in range(n_adds):
        stacked.add()
        frames.add(stream["ages"][k])
    return stacked, frames


def stacked_stores(model, stream):
    """The numpy stores a stacked host replay buffer holds after the model's adds: (stores, next_stores or None, scalars) for
    replay_cases.sample_reference; slots never written hold zeros."""
    T = model.T

    def held(tag, key):
        if tag is None:
            return np.zeros_like(stream["obs"][key][0])
        return (stream["obs"] if tag[0] == "obs" else stream["next_obs"])[key][tag[1]]

    stores = {key: np.stack([held(model.obs[t], key) for t in range(T)]) for key in stream["obs"]}
    nstores = None if model.single_store else {key: np.stack([held(model.next_obs[t], key) for t in range(T)]) for key in stream["obs"]}
    ks = [model.step[t] if model.step[t] is not None else 0 for t in range(T)]
    scalars = dict(actions=stream["actions"][ks], rewards=stream["rewards"][ks], dones=stream["dones"][ks].astype(np.float32),
                   timeouts=None if model.single_store else stream["timeouts"][ks].astype(np.float32))
    return stores, nstores, scalars


def expected_from_model(model, stream, t, e, image_normalization=(0, 1), tactile_normalization=(-1, 1)):
    """(observations, next_observations) of steps (t, e) by the restated rule: the stacks put together from the newest frames the model's slots
    hold, through the reference's flatten and vt_load (rollout_cases)."""
    def frame(tag, key, env):
        return (stream["obs"] if tag[0] == "obs" else stream["next_obs"])[key][tag[1], env, -1]

    out = []
    for tags_of in (model.obs_frames, model.next_frames):
        picked = {key: np.stack([np.stack([frame(tag, key, ee) for tag in tags_of(tt, ee)]) for tt, ee in zip(t, e)]) for key in stream["obs"]}
        out.append(RC.vt_load_reference(RC.flatten_frame_stack(picked), model.fs, image_normalization, tactile_normalization))
    return out


def frames_reference(frames, next_frames, ages, rows, fs, image_normalization=(0, 1), tactile_normalization=(-1, 1)):
    """m3l_replay_gather_load_frames restated on numpy frame stores {'image': (T, n_envs, H, W, 3), 'tactile': (T, n_envs, 3 S, h, w)}
    (next_frames None: the single-store mode), ages (T, n_envs) of any integers — clamped to [0, fs - 1] — and valid rows t * n_envs + e."""
    first = next(iter(frames.values()))
    T, n_envs = first.shape[:2]
    rows = np.asarray(rows, dtype=np.int64)
    t, e = rows // n_envs, rows % n_envs
    a = np.clip(np.asarray(ages)[t, e], 0, fs - 1)
    back = [np.minimum(fs - 1 - j, a) for j in range(fs)]
    out = []
    obs = {k: np.stack([v[(t - back[j]) % T, e] for j in range(fs)], axis=1) for k, v in frames.items()}
    newest = {k: (v[(t + 1) % T, e] if next_frames is None else next_frames[k][t, e]) for k, v in frames.items()}
    nxt = {k: np.concatenate([obs[k][:, 1:], newest[k][:, None]], axis=1) for k in frames}
    for picked in (obs, nxt):
        out.append(RC.vt_load_reference(RC.flatten_frame_stack(picked), fs, image_normalization, tactile_normalization))
    return out


def make_frame_stores(T, n_envs, image_hw, tactile_hw, S, image_dtype, tactile_dtype, seed):
    """Seeded frame stores for the direct calls: rollout_cases.make_stores with one frame per slot, the fs axis dropped."""
    return {k: v[:, :, 0] for k, v in RC.make_stores(T, n_envs, 1, image_hw, tactile_hw, S, image_dtype, tactile_dtype, seed).items()}
