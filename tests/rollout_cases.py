"""Restatements and inputs for the rollout tests (test_rollout_cpu.py, test_rollout_gpu.py, golden/make_golden_rollout.py).

`feed_reference` restates, in numpy, what the reference does between its rollout buffer and `self.mae(x)` (models/ppo_dino_cat_mae.py):
swap_and_flatten :25-29, `obs[idx]` :48-56, the frame-stack permute / reshape :295-301, and vt_load (utils/pretrain_utils.py:7-57), whose
arithmetic is float32: `torch.Tensor(x) - lo` rounds lo to float32, `/ (hi - lo)` forms the span in double and rounds it once.  numpy's float32
subtraction and division are the same IEEE operations, so this is held to tests/golden/rollout_feed.npz bit for bit.

`gae_reference` restates stable-baselines3's `RolloutBuffer.compute_returns_and_advantage` in float64.  SB3 is not in the reference tree, so
nothing pins it (parity unpinned); the hand-computed cases of test_rollout_cpu.py hold the restatement itself.
"""
import numpy as np


def flat_to_row(j, T, n_envs):
    """Flat index of the reference's swapped order -> (t, env): swap_and_flatten turns (T, n_envs, ...) into (n_envs * T, ...), env-major."""
    return j % T, j // T


def swap_and_flatten(arr):
    """models/ppo_dino_cat_mae.py:25-29."""
    shape = arr.shape
    if len(shape) < 3:
        shape = (*shape, 1)
    return arr.swapaxes(0, 1).reshape(shape[0] * shape[1], *shape[2:])


def flatten_frame_stack(obs):
    """:295-301 on numpy arrays: image (B, fs, H, W, 3) -> (B, H, W, 3 fs); tactile (B, fs, 3 S, h, w) -> (B, 3 S fs, h, w)."""
    out = dict(obs)
    if "image" in out:
        im = out["image"].transpose(0, 2, 3, 1, 4)
        out["image"] = im.reshape(im.shape[0], im.shape[1], im.shape[2], -1)
    if "tactile" in out:
        t = out["tactile"]
        out["tactile"] = t.reshape(t.shape[0], -1, t.shape[3], t.shape[4])
    return out


def vt_load_reference(obs, frame_stack, image_normalization=(0, 1), tactile_normalization=(-1, 1)):
    """utils/pretrain_utils.py:7-57 on flattened numpy observations, float32 arithmetic."""
    out = {}
    if "image" in obs:
        lo, hi = image_normalization
        x = obs["image"].astype(np.float32).transpose(0, 3, 1, 2)
        out["image"] = np.ascontiguousarray((x - np.float32(lo)) / np.float32(float(hi) - float(lo)))
    if "tactile" in obs:
        lo, hi = tactile_normalization
        n_tactiles = obs["tactile"].shape[1] // frame_stack
        pick = np.array([i * n_tactiles + c for i in range(frame_stack) for c in range(3)])
        for s in range(n_tactiles // 3):
            x = obs["tactile"][:, pick + 3 * s].astype(np.float32)
            out["tactile" + str(s + 1)] = np.ascontiguousarray((x - np.float32(lo)) / np.float32(float(hi) - float(lo)))
    return out


def feed_reference(stores, idx, image_normalization=(0, 1), tactile_normalization=(-1, 1)):
    """stores {'image': (T, n_envs, fs, H, W, 3), 'tactile': (T, n_envs, fs, 3 S, h, w)} (either key), idx: flat indices -> the MAE's input."""
    idx = np.asarray(idx, dtype=np.int64)
    picked = {k: swap_and_flatten(v)[idx] for k, v in stores.items()}
    fs = next(iter(stores.values())).shape[2]
    return vt_load_reference(flatten_frame_stack(picked), fs, image_normalization, tactile_normalization)


def gae_reference(rewards, values, episode_starts, last_values, dones, gamma, gae_lambda):
    """SB3 RolloutBuffer.compute_returns_and_advantage in float64: (T, n_envs) arrays, last_values / dones (n_envs) -> advantages, returns."""
    rewards, values, episode_starts = (np.asarray(a, dtype=np.float64) for a in (rewards, values, episode_starts))
    last_values, dones = np.asarray(last_values, dtype=np.float64), np.asarray(dones, dtype=np.float64)
    T = rewards.shape[0]
    adv = np.zeros_like(rewards)
    last_gae_lam = 0.0
    for step in reversed(range(T)):
        if step == T - 1:
            next_non_terminal, next_values = 1.0 - dones, last_values
        else:
            next_non_terminal, next_values = 1.0 - episode_starts[step + 1], values[step + 1]
        delta = rewards[step] + gamma * next_values * next_non_terminal - values[step]
        last_gae_lam = delta + gamma * gae_lambda * next_non_terminal * last_gae_lam
        adv[step] = last_gae_lam
    return adv, adv + values


def make_stores(T, n_envs, fs, image_hw, tactile_hw, S, image_dtype, tactile_dtype, seed):
    """Seeded observation stores in the vec-env's layout; image_hw / tactile_hw None leaves that key out.  uint8 stores cover 0..255, float
    images [0, 1), float tactile frames [-1, 1)."""
    g = np.random.default_rng(seed)
    stores = {}
    if image_hw is not None:
        shape = (T, n_envs, fs, image_hw[0], image_hw[1], 3)
        stores["image"] = g.integers(0, 256, shape, dtype=np.uint8) if np.dtype(image_dtype) == np.uint8 else g.random(shape, dtype=np.float32)
    if tactile_hw is not None:
        shape = (T, n_envs, fs, 3 * S, tactile_hw[0], tactile_hw[1])
        stores["tactile"] = g.integers(0, 256, shape, dtype=np.uint8) if np.dtype(tactile_dtype) == np.uint8 else \
            (2 * g.random(shape, dtype=np.float32) - 1).astype(np.float32)
    return stores


def make_scalars(T, n_envs, A, seed, starts="random", dones="random"):
    """Seeded per-step scalars: actions (T, n_envs, A), rewards / values / log_probs / episode_starts (T, n_envs), last_values / dones (n_envs)."""
    g = np.random.default_rng(seed)
    f = lambda *s: g.standard_normal(s).astype(np.float32)      # noqa: E731
    es = (g.random((T, n_envs)) < 0.3).astype(np.float32) if starts == "random" else np.zeros((T, n_envs), np.float32)
    es[0] = 1.0
    if T > 2:
        es[T // 2, 0] = 1.0                                     # an episode start inside the rollout, whatever the draw
    d = (g.random(n_envs) < 0.5).astype(np.float32) if dones == "random" else np.zeros(n_envs, np.float32)
    d[-1] = 1.0                                                 # a `done` at the rollout's end
    return dict(actions=f(T, n_envs, A), rewards=f(T, n_envs), values=f(T, n_envs), log_probs=f(T, n_envs), episode_starts=es,
                last_values=f(n_envs), dones=d)


# the golden's dimensions (golden/make_golden_rollout.py): T = 3, n_envs = 2, fs = 2, image 8 x 8, 2 sensors at 4 x 4
GOLDEN = dict(T=3, n_envs=2, fs=2, image_hw=(8, 8), tactile_hw=(4, 4), S=2)
GOLDEN_INDEX_LISTS = [[0, 5, 2, 2, 4], [5], [3, 0, 1, 5, 5, 0, 2]]        # repeated, first (0) and last (T n_envs - 1 = 5) indices
GOLDEN_VARIANTS = {"u8": (np.uint8, 101, (0, 255), (-2, 3)), "f32": (np.float32, 102, (0, 1), (-1, 1))}   # image dtype, seed, ranges
