"""CPU-only checks of the device-resident rollout (m3l_amd/rollout.py, csrc/rollout.hip): the numpy / float64 restatements of
tests/rollout_cases.py against the reference's recorded minibatches and against hand-computed cases, and every rejection of the public
surface.  No kernel is launched here: the C entry points are reached only with arguments they refuse before any launch."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import m3l_amd
import rollout_cases as RC
from m3l_amd import _lib as L
from m3l_amd import rollout as R


@pytest.fixture(scope="module")
def golden(golden_dir):
    return np.load(os.path.join(golden_dir, "rollout_feed.npz"))


def test_exports_and_abi():
    assert L.lib().m3l_version() >= 411
    for name in ("m3l_rollout_gather_load", "m3l_rollout_gather_rows", "m3l_rollout_gae"):
        assert name in L.EXPORTS
    for name in ("DeviceRolloutBuffer", "LoadedObs", "RolloutBatch"):
        assert name in m3l_amd.__all__ and hasattr(m3l_amd, name)
    assert issubclass(R.LoadedObs, dict) and m3l_amd.pretrain_utils.LoadedObs is R.LoadedObs


@pytest.mark.parametrize("variant", sorted(RC.GOLDEN_VARIANTS))
def test_restatement_reproduces_the_reference(golden, variant):
    """swap_and_flatten -> obs[idx] -> collate -> reshape -> vt_load as the reference ran them, against the numpy restatement: equal bits."""
    image_dtype, _, img_range, tac_range = RC.GOLDEN_VARIANTS[variant]
    stores = {k: golden[f"{variant}/store/{k}"] for k in ("image", "tactile")}
    assert stores["image"].dtype == image_dtype and stores["image"].shape == (3, 2, 2, 8, 8, 3) and stores["tactile"].shape == (3, 2, 2, 6, 4, 4)
    assert tuple(golden[f"{variant}/ranges"]) == tuple(map(float, img_range + tac_range))
    for i, idx in enumerate(RC.GOLDEN_INDEX_LISTS):
        assert golden[f"{variant}/idx{i}"].tolist() == idx
        x = RC.feed_reference(stores, idx, img_range, tac_range)
        assert sorted(x) == ["image", "tactile1", "tactile2"]
        for k, v in x.items():
            want = golden[f"{variant}/out{i}/x/{k}"]
            assert v.dtype == np.float32 and v.shape == want.shape
            np.testing.assert_array_equal(v, want, err_msg=f"{variant} list {i} {k}")
        for k, out in (("actions", "actions"), ("values", "old_values"), ("log_probs", "old_log_prob"), ("advantages", "advantages"), ("returns", "returns")):
            got = RC.swap_and_flatten(golden[f"{variant}/store/{k}"])[np.asarray(idx)]
            np.testing.assert_array_equal(got if k == "actions" else got.reshape(-1), golden[f"{variant}/out{i}/{out}"])
    assert {0, 5} <= set(sum(RC.GOLDEN_INDEX_LISTS, [])) and any(len(set(l)) < len(l) for l in RC.GOLDEN_INDEX_LISTS)


def test_flat_index_map_is_the_swapped_order():
    """T != n_envs: flat index j addresses (t, env) = (j % T, j // T); the un-swapped t * n_envs + env differs."""
    T, E = 5, 3
    arr = np.arange(T * E).reshape(T, E)                  # arr[t, env] = t * E + env
    flat = RC.swap_and_flatten(arr)[:, 0]
    unswapped_hits = 0
    for j in range(T * E):
        t, env = RC.flat_to_row(j, T, E)
        assert flat[j] == arr[t, env] == t * E + env
        assert (t, env) == (j % T, j // T)
        unswapped_hits += int(flat[j] == j)
    assert unswapped_hits < T * E                         # reading row j itself (no swap) would be wrong for most j
    stores = RC.make_stores(T, E, 1, (2, 2), None, 0, np.float32, None, 7)
    x = RC.feed_reference(stores, list(range(T * E)))["image"]
    for j in range(T * E):
        t, env = RC.flat_to_row(j, T, E)
        np.testing.assert_array_equal(x[j], stores["image"][t, env, 0].transpose(2, 0, 1))


def test_gae_restatement_by_hand():
    g, lam = 0.9, 0.8
    # T = 1: A = r + g v_last (1 - done) - v
    adv, ret = RC.gae_reference([[1.0, 2.0]], [[0.5, -1.0]], [[1.0, 1.0]], [3.0, 4.0], [0.0, 1.0], g, lam)
    np.testing.assert_allclose(adv, [[1.0 + g * 3.0 - 0.5, 2.0 + 1.0]], rtol=0, atol=1e-15)
    np.testing.assert_allclose(ret, adv + np.array([[0.5, -1.0]]), rtol=0, atol=1e-15)
    # T = 3, one environment, an episode start at t = 1: step 0 sees neither v_1 nor A_1
    r, v, lv = [1.0, 2.0, 3.0], [0.1, 0.2, 0.3], 0.4
    adv, ret = RC.gae_reference(np.array(r)[:, None], np.array(v)[:, None], [[1.0], [1.0], [0.0]], [lv], [0.0], g, lam)
    a2 = r[2] + g * lv - v[2]
    a1 = r[1] + g * v[2] - v[1] + g * lam * a2
    a0 = r[0] - v[0]
    np.testing.assert_allclose(adv[:, 0], [a0, a1, a2], rtol=0, atol=1e-15)
    np.testing.assert_allclose(ret[:, 0], [a0 + v[0], a1 + v[1], a2 + v[2]], rtol=0, atol=1e-15)
    # no episode start inside: the full recurrence; gamma = lambda = 1 telescopes to sum r + v_last - v_t (another order of the same float64
    # sums: a handful of roundings at magnitude < 8, ulp 8.9e-16)
    adv, _ = RC.gae_reference(np.array(r)[:, None], np.array(v)[:, None], [[1.0], [0.0], [0.0]], [lv], [0.0], 1.0, 1.0)
    np.testing.assert_allclose(adv[:, 0], [6.0 + lv - v[0], 5.0 + lv - v[1], 3.0 + lv - v[2]], rtol=0, atol=1e-14)


SHAPES = {"image": (2, 8, 8, 3), "tactile": (2, 6, 4, 4)}
DTYPES = {"image": np.uint8, "tactile": np.float32}


def _buffer(**kw):
    args = dict(buffer_size=3, n_envs=2, obs_shapes=SHAPES, obs_dtypes=DTYPES, action_dim=3)
    args.update(kw)
    return m3l_amd.DeviceRolloutBuffer(**args)


def test_constructor_touches_no_device_and_keeps_sb3_surface():
    buf = _buffer()
    assert (buf.pos, buf.full, buf.frame_stack, buf.gamma, buf.gae_lambda) == (0, False, 2, 0.99, 0.95)
    assert buf.obs_dtypes == {"image": torch.uint8, "tactile": torch.float32}
    for name in ("reset", "add", "compute_returns_and_advantage", "get"):
        assert callable(getattr(buf, name))


def test_cpu_placement_is_refused():
    with pytest.raises(m3l_amd.M3LError, match="no CPU fallback"):
        _buffer(device="cpu")
    idx = torch.zeros(2, dtype=torch.int64)
    with pytest.raises(m3l_amd.M3LError, match="must live on the GPU"):
        R.gather_load(torch.zeros(3, 2, 1, 4, 4, 3), None, idx)
    with pytest.raises(m3l_amd.M3LError, match="must live on the GPU"):
        R.gather_rows(torch.zeros(3, 2, 1), *[torch.zeros(3, 2) for _ in range(4)], idx)
    with pytest.raises(m3l_amd.M3LError, match="must live on the GPU"):
        R.gae(*[torch.zeros(3, 2) for _ in range(3)], torch.zeros(2), torch.zeros(2), 0.99, 0.95)


@pytest.mark.parametrize("dt", [np.float64, np.int8, np.float16, torch.bfloat16, "int32"])
def test_observation_dtypes_other_than_uint8_and_float32_are_refused(dt):
    with pytest.raises(ValueError, match="uint8 or float32"):
        _buffer(obs_dtypes={"image": dt, "tactile": np.float32})
    with pytest.raises(ValueError, match="uint8 or float32"):
        _buffer(obs_dtypes={"image": np.uint8, "tactile": dt})


@pytest.mark.parametrize("channels", [4, 7, 27, 0])
def test_tactile_channel_count_must_be_3s(channels):
    with pytest.raises(ValueError, match=r"3 \* S"):
        _buffer(obs_shapes={"image": (2, 8, 8, 3), "tactile": (2, channels, 4, 4)})


def test_other_constructor_rejections():
    with pytest.raises(ValueError, match="frame_stack, H, W, 3"):
        _buffer(obs_shapes={"image": (2, 8, 8, 4), "tactile": (2, 6, 4, 4)})
    with pytest.raises(ValueError, match="frame stack"):
        _buffer(obs_shapes={"image": (2, 8, 8, 3), "tactile": (4, 6, 4, 4)})
    with pytest.raises(ValueError, match="observation keys"):
        _buffer(obs_shapes={"depth": (2, 8, 8, 3)}, obs_dtypes={"depth": np.uint8})
    with pytest.raises(ValueError, match="empty image normalisation range"):
        _buffer(image_normalization=[1, 1])
    with pytest.raises(ValueError, match="empty tactile normalisation range"):
        _buffer(tactile_normalization=[0.5, 0.5])
    with pytest.raises(ValueError, match="must be positive"):
        _buffer(buffer_size=0)


def test_get_before_full_and_add_when_full_are_refused():
    buf = _buffer()
    with pytest.raises(ValueError, match="not full"):
        buf.get(batch_size=4)                              # raised by the call itself, not by the first next()
    with pytest.raises(ValueError, match="steps stored"):
        buf.compute_returns_and_advantage(torch.zeros(2), np.zeros(2, bool))
    buf.pos, buf.full = buf.buffer_size, True              # as after buffer_size add() calls (which need the GPU)
    obs = {"image": np.zeros((2,) + SHAPES["image"], np.uint8), "tactile": np.zeros((2,) + SHAPES["tactile"], np.float32)}
    with pytest.raises(ValueError, match="full"):
        buf.add(obs, np.zeros((2, 3), np.float32), np.zeros(2, np.float32), np.zeros(2, bool), torch.zeros(2), torch.zeros(2))
    for bad in ([0, 6], [-1], [], [[0, 1]], [0.5]):
        with pytest.raises(ValueError, match="indices"):
            buf.get(batch_size=4, indices=bad)
    buf.reset()
    assert (buf.pos, buf.full) == (0, False)
    with pytest.raises(ValueError, match="shape"):
        buf.add({"image": obs["image"][:1], "tactile": obs["tactile"]}, None, None, None, None, None)
    with pytest.raises(ValueError, match="observation keys"):
        buf.add({"image": obs["image"]}, None, None, None, None, None)


def _gather_load_rc(**kw):
    """m3l_rollout_gather_load with arguments it must refuse before any launch (the pointers are never dereferenced on the host)."""
    a = dict(image=1 << 20, image_u8=0, H=8, W=8, img=(0.0, 1.0), image_out=1 << 21, tactile=1 << 22, tactile_u8=0, th=4, tw=4, S=2, tac=(-1.0, 1.0),
             T=3, n_envs=2, fs=2, idx=1 << 23, B=4)
    a.update(kw)
    outs = (C.c_void_p * 16)(*([1 << 24] * 16))
    return L.lib().m3l_rollout_gather_load(a["image"], a["image_u8"], a["H"], a["W"], a["img"][0], a["img"][1], a["image_out"], a["tactile"], a["tactile_u8"],
                                           a["th"], a["tw"], a["S"], a["tac"][0], a["tac"][1], outs, a["T"], a["n_envs"], a["fs"], a["idx"], a["B"], None)


@pytest.mark.parametrize("kw,msg", [
    (dict(S=0), "n_sensors=0"), (dict(S=9), "n_sensors=9"), (dict(img=(0.25, 0.25)), "empty image normalisation range"),
    (dict(tac=(1.0, 1.0)), "empty tactile normalisation range"), (dict(image=None, tactile=None), "neither an image nor a tactile store"),
    (dict(B=0), "B=0"), (dict(T=0), "T=0"), (dict(H=0), "image H=0"),
])
def test_entry_point_rejections_before_any_launch(kw, msg):
    assert _gather_load_rc(**kw) == 1
    assert msg in L.last_error()


def test_rows_and_gae_entry_points_refuse_bad_sizes():
    lib = L.lib()
    p = 1 << 20
    assert lib.m3l_rollout_gather_rows(p, p, p, p, p, 3, 2, 0, p, 4, p, p, p, p, p, None) == 1 and "A=0" in L.last_error()
    assert lib.m3l_rollout_gather_rows(p, p, p, p, p, 3, 2, 2, p, 0, p, p, p, p, p, None) == 1 and "B=0" in L.last_error()
    assert lib.m3l_rollout_gather_rows(p, None, p, p, p, 3, 2, 2, p, 4, p, p, p, p, p, None) == 1 and "NULL" in L.last_error()
    assert lib.m3l_rollout_gae(p, p, p, p, p, 0, 2, 0.99, 0.95, p, p, None) == 1 and "T=0" in L.last_error()
    assert lib.m3l_rollout_gae(p, p, p, None, p, 3, 2, 0.99, 0.95, p, p, None) == 1 and "NULL" in L.last_error()


def test_extractors_take_loaded_observations_as_they_are(monkeypatch):
    """A LoadedObs skips the frame-stack flatten and vt_load; any other mapping takes today's path."""
    from m3l_amd import fusion
    calls = []
    monkeypatch.setattr(fusion, "vt_load", lambda obs, frame_stack, device: calls.append(("vt_load", frame_stack)) or {"from": "vt_load"})
    x = R.LoadedObs(image=torch.zeros(1, 6, 8, 8))
    assert fusion._loaded(x, 2, "cpu") is x and calls == []
    assert fusion._loaded({"image": torch.zeros(1, 2, 8, 8, 3)}, 2, "cpu") == {"from": "vt_load"} and calls == [("vt_load", 2)]
    assert fusion._loaded(dict(x), 2, "cpu") == {"from": "vt_load"}          # a plain dict of the same tensors is not trusted to be loaded
