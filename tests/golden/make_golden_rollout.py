#!/usr/bin/env python3
"""Golden minibatches of the reference's rollout feed, recorded from the reference's own code (runs only where /root/reference is mounted).

`models/ppo_dino_cat_mae.py` is imported from where it lies with the inert stubs make_golden_ppo_head.py uses for its non-arithmetic imports
(gymnasium, stable_baselines3.*), and `utils/pretrain_utils.py` as the file it is (cv2, tqdm and SB3's logger stubbed).  On a duck-typed rollout
buffer of T = 3 steps, n_envs = 2, frame_stack = 2, image 8 x 8, 2 tactile sensors at 4 x 4 (tests/rollout_cases.py GOLDEN) the reference's own
functions run in the order `PPO_MAE.train` runs them:

  RolloutDataset(buffer)           -> prepare(): swap_and_flatten of the observations and the five per-step arrays          :31-46, :25-29
  dataset[j] for j in a fixed list -> __getitem__                                                                            :48-56
  torch's default_collate          what DataLoader(dataset, batch_size) applies to the samples                               :269
  the three reshape lines          :295-301 sit inside `train`; restated here, as m3l_amd.fusion._flatten_frame_stack does
  vt_load(observations, frame_stack=fs, <ranges>)                                                                            utils/pretrain_utils.py:7-57

Two variants: a uint8 image store with the ranges [0, 255] / [-2, 3] of vt_load_u8.npz, and a float32 one with the defaults.  The index lists
hold a repeated index, index 0 and the last index.  The file holds the stores as the vec-env filled them, the per-step arrays, the index lists,
and per list the loaded observations and the gathered per-step arrays: data only.

Usage:  python tests/golden/make_golden_rollout.py        (rewrites tests/golden/rollout_feed.npz)
"""
import importlib.util
import os
import sys
import types

import numpy as np
import torch
from torch.utils.data import default_collate

HERE = os.path.dirname(os.path.abspath(__file__))
REF = "/root/reference"
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)
import rollout_cases as RC  # noqa: E402
from make_golden_ppo_head import _install_stubs  # noqa: E402


def _load_reference():
    _install_stubs()

    class _Dummy:
        def __init__(self, *a, **k):
            pass
    for name, attrs in (("cv2", {}), ("tqdm", {"tqdm": lambda it, **k: it}), ("stable_baselines3.common.logger", {"Video": _Dummy})):
        m = types.ModuleType(name)
        m.__dict__.update(attrs)
        sys.modules[name] = m

    def load(name, path):
        spec = importlib.util.spec_from_file_location(name, os.path.join(REF, path))
        m = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(m)
        return m
    pu = load("utils.pretrain_utils", "utils/pretrain_utils.py")      # the reference's own vt_load, in place of the stub
    sys.modules["utils.pretrain_utils"] = pu
    sys.modules["utils"].pretrain_utils = pu
    return load("ref_ppo_dino_cat_mae", "models/ppo_dino_cat_mae.py"), pu


def _flatten(obs):
    """What :295-301 do to a collated batch: image (B, fs, H, W, 3) -> (B, H, W, 3 fs), tactile (B, fs, C, h, w) -> (B, fs C, h, w)."""
    obs, fs = dict(obs), 1
    if "image" in obs and obs["image"].dim() == 5:
        B, fs, H, W, _ = obs["image"].shape
        obs["image"] = obs["image"].permute(0, 2, 3, 1, 4).reshape(B, H, W, -1)
    if "tactile" in obs and obs["tactile"].dim() == 5:
        B, fs, _, h, w = obs["tactile"].shape
        obs["tactile"] = obs["tactile"].reshape(B, -1, h, w)
    return obs, fs


def run_variant(ref, pu, name):
    image_dtype, seed, img_range, tac_range = RC.GOLDEN_VARIANTS[name]
    G = RC.GOLDEN
    stores = RC.make_stores(G["T"], G["n_envs"], G["fs"], G["image_hw"], G["tactile_hw"], G["S"], image_dtype, np.float32, seed)
    sc = RC.make_scalars(G["T"], G["n_envs"], 3, seed + 50)
    adv, ret = (a.astype(np.float32) for a in RC.gae_reference(sc["rewards"], sc["values"], sc["episode_starts"], sc["last_values"], sc["dones"], 0.99, 0.95))
    z = {f"{name}/store/{k}": v for k, v in stores.items()}
    per_step = dict(actions=sc["actions"], values=sc["values"], log_probs=sc["log_probs"], advantages=adv, returns=ret)
    z.update({f"{name}/store/{k}": v for k, v in per_step.items()})
    buf = types.SimpleNamespace(buffer_size=G["T"], n_envs=G["n_envs"], observations={k: v.copy() for k, v in stores.items()},
                                **{k: v.copy() for k, v in per_step.items()})
    dataset = ref.RolloutDataset(buf)                       # prepare() swaps and flattens in place
    assert len(dataset) == G["T"] * G["n_envs"]
    for i, idx in enumerate(RC.GOLDEN_INDEX_LISTS):
        batch = default_collate([dataset[j] for j in idx])
        observations, frame_stack = _flatten(batch["observations"])
        x = pu.vt_load(dict(observations), image_normalization=list(img_range), tactile_normalization=list(tac_range), frame_stack=frame_stack)
        z[f"{name}/idx{i}"] = np.asarray(idx, dtype=np.int64)
        for k, v in x.items():
            assert v.dtype == torch.float32
            z[f"{name}/out{i}/x/{k}"] = v.numpy()
        for k_ref, k_out in (("actions", "actions"), ("old_values", "old_values"), ("old_log_prob", "old_log_prob"), ("advantages", "advantages"),
                             ("returns", "returns")):
            v = batch[k_ref]
            z[f"{name}/out{i}/{k_out}"] = (v if k_ref == "actions" else v.flatten()).numpy()       # cuda_flatten_preprocess :58-62
    z[f"{name}/ranges"] = np.array(list(img_range) + list(tac_range), dtype=np.float64)
    return z


def main():
    ref, pu = _load_reference()
    z = {}
    for name in RC.GOLDEN_VARIANTS:
        z.update(run_variant(ref, pu, name))
    path = os.path.join(HERE, "rollout_feed.npz")
    np.savez_compressed(path, **z)
    print("wrote", path, os.path.getsize(path), "bytes,", len(z), "arrays")


if __name__ == "__main__":
    main()
