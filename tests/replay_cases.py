"""Restatements and inputs for the replay-buffer tests (test_replay_cpu.py, test_replay_gpu.py).

stable-baselines3 is not in the reference tree, so its `DictReplayBuffer` (and `ReplayBuffer`'s optimize_memory_usage mode) is restated here
from its documented behaviour and nothing pins the restatement (parity unpinned); the hand-computed cases of test_replay_cpu.py hold it.  The
observation path is the reference's own — the frame-stack permute models/sac_mae.py:253-260 and vt_load — and reuses the numpy restatement of
rollout_cases.py, which tests/golden/rollout_feed.npz pins bit for bit.

`sample_reference`   what `sample()` returns for given (batch_inds, env_indices): numpy fancy indexing of the stores, the next observation from
                     the second store or from step (t + 1) % T of the single store, dones * (1 - timeouts), VecNormalize's reward normalisation
`RingModel`          add / pos / full of the ring in pure Python, which step every slot holds, and the steps a sample may come from
"""
import math

import numpy as np

import rollout_cases as RC


def normalize_reward_reference(rewards, var, epsilon, clip, dtype=np.float32):
    """VecNormalize.normalize_reward: clip(r / sqrt(var + epsilon), -clip, clip).  dtype float32: the scale is formed in double and rounded once,
    the division and the clip are IEEE float32 (what the kernel computes); dtype float64: the exact value to hold the float32 one against."""
    s = math.sqrt(float(var) + float(epsilon))
    r = np.asarray(rewards, dtype=dtype)
    return np.clip(r / dtype(s), dtype(-clip), dtype(clip))


def sample_reference(stores, next_stores, scalars, batch_inds, env_indices, T, reward_norm=None, image_normalization=(0, 1),
                     tactile_normalization=(-1, 1)):
    """stores / next_stores {'image': (T, n_envs, fs, H, W, 3), 'tactile': (T, n_envs, fs, 3 S, h, w)} (next_stores None: the single-store mode),
    scalars {'actions': (T, n_envs, A), 'rewards', 'dones', 'timeouts' (optional): (T, n_envs)}, reward_norm None or (var, epsilon, clip)
    -> dict(observations, next_observations: the MAE's inputs; actions (B, A); dones, rewards (B, 1); rows (B))."""
    t, e = np.asarray(batch_inds, dtype=np.int64), np.asarray(env_indices, dtype=np.int64)
    first = next(iter(stores.values()))
    assert first.shape[0] == T
    n_envs, fs = first.shape[1], first.shape[2]

    def load(picked):
        return RC.vt_load_reference(RC.flatten_frame_stack(picked), fs, image_normalization, tactile_normalization)

    obs = load({k: v[t, e] for k, v in stores.items()})
    if next_stores is None:
        nxt = load({k: v[(t + 1) % T, e] for k, v in stores.items()})
    else:
        nxt = load({k: v[t, e] for k, v in next_stores.items()})
    dones = scalars["dones"][t, e].astype(np.float32)
    if scalars.get("timeouts") is not None:
        dones = dones * (np.float32(1) - scalars["timeouts"][t, e].astype(np.float32))
    rewards = scalars["rewards"][t, e].astype(np.float32)
    if reward_norm is not None:
        rewards = normalize_reward_reference(rewards, *reward_norm)
    return dict(observations=obs, next_observations=nxt, actions=scalars["actions"][t, e], dones=dones.reshape(-1, 1), rewards=rewards.reshape(-1, 1),
                rows=t * n_envs + e)


class RingModel:
    """SB3's ring in pure Python.  `obs[slot]` / `next_obs[slot]` name what the slot holds as ('obs' | 'next', k) for the k-th add (None: never
    written); in the single-store mode next observations go to the following slot of `obs` and `next_obs` stays None."""

    def __init__(self, T, single_store=False):
        self.T, self.single_store = T, single_store
        self.pos, self.full, self.n_adds = 0, False, 0
        self.obs = [None] * T
        self.next_obs = None if single_store else [None] * T
        self.step = [None] * T                      # which add's action / reward / done the slot holds

    def add(self):
        k, p = self.n_adds, self.pos
        self.obs[p] = ("obs", k)
        if self.single_store:
            self.obs[(p + 1) % self.T] = ("next", k)
        else:
            self.next_obs[p] = ("next", k)
        self.step[p] = k
        self.n_adds += 1
        self.pos += 1
        if self.pos == self.T:
            self.full, self.pos = True, 0

    def size(self):
        return self.T if self.full else self.pos

    def next_of(self, t):
        """What a sample of step t reads as its next observation."""
        return self.obs[(t + 1) % self.T] if self.single_store else self.next_obs[t]

    def valid_steps(self):
        if self.single_store and self.full:
            return [(u + self.pos) % self.T for u in range(1, self.T)]
        return list(range(self.size()))


def make_replay_scalars(T, n_envs, A, seed):
    """Seeded actions (T, n_envs, A), rewards in about [-6, 6], dones and timeouts (0 / 1) with every combination present when T n_envs >= 4:
    (done, timeout) = (1, 1) at [0, 0], (1, 0) at [-1, -1], (0, 0) and (0, 1) elsewhere (a timeout without a done does not occur in SB3 and
    must not matter: 0 * (1 - 1) = 0)."""
    g = np.random.default_rng(seed)
    actions = g.standard_normal((T, n_envs, A)).astype(np.float32)
    rewards = (3 * g.standard_normal((T, n_envs))).astype(np.float32)
    dones = (g.random((T, n_envs)) < 0.4).astype(np.float32)
    timeouts = (dones * (g.random((T, n_envs)) < 0.5)).astype(np.float32)
    dones[0, 0] = timeouts[0, 0] = 1.0
    dones[-1, -1], timeouts[-1, -1] = 1.0, 0.0
    return dict(actions=actions, rewards=rewards, dones=dones, timeouts=timeouts)
