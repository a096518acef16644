"""CPU-only checks of the device-resident replay buffer (m3l_amd/replay.py, csrc/replay.hip): the numpy restatements of tests/replay_cases.py
against the reference's recorded minibatches and against hand-computed cases, and every rejection of the public surface.  No kernel is launched
here: the C entry points are reached only with arguments they refuse before any launch."""
import ctypes as C
import math
import os
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import m3l_amd
import replay_cases as PC
import rollout_cases as RC
from m3l_amd import _lib as L
from m3l_amd import replay as P
from m3l_amd import rollout as R


@pytest.fixture(scope="module")
def golden(golden_dir):
    return np.load(os.path.join(golden_dir, "rollout_feed.npz"))


def test_exports_and_abi():
    assert L.lib().m3l_version() >= 412
    for name in ("m3l_replay_gather_load", "m3l_replay_gather_rows"):
        assert name in L.EXPORTS
    for name in ("DeviceReplayBuffer", "ReplayBatch"):
        assert name in m3l_amd.__all__ and hasattr(m3l_amd, name)
    assert m3l_amd.ReplayBatch._fields == ("observations", "actions", "next_observations", "dones", "rewards", "rows")
    # the validation is the rollout's own code, not a copy of it
    assert P._obs_spec is R._obs_spec and P._check_obs is R._check_obs


@pytest.mark.parametrize("variant", sorted(RC.GOLDEN_VARIANTS))
def test_restatement_reproduces_the_reference(golden, variant):
    """The reference's recorded minibatches were drawn with flat indices j of its swapped order; row (j % T) * n_envs + j // T of the un-swapped
    store is the same transition, so the restated `observations` of those (t, e) equal the recorded MAE inputs bit for bit: this pins the row map
    t * n_envs + e and the load to the reference's own run."""
    _, _, img_range, tac_range = RC.GOLDEN_VARIANTS[variant]
    T, E = RC.GOLDEN["T"], RC.GOLDEN["n_envs"]
    stores = {k: golden[f"{variant}/store/{k}"] for k in ("image", "tactile")}
    scalars = dict(actions=golden[f"{variant}/store/actions"], rewards=golden[f"{variant}/store/values"], dones=np.zeros((T, E), np.float32))
    for i, idx in enumerate(RC.GOLDEN_INDEX_LISTS):
        j = np.asarray(idx)
        got = PC.sample_reference(stores, None, scalars, j % T, j // T, T, None, img_range, tac_range)
        assert got["rows"].tolist() == [(x % T) * E + x // T for x in idx]
        assert sorted(got["observations"]) == ["image", "tactile1", "tactile2"]
        for k, v in got["observations"].items():
            want = golden[f"{variant}/out{i}/x/{k}"]
            assert v.dtype == np.float32 and v.shape == want.shape
            np.testing.assert_array_equal(v, want, err_msg=f"{variant} list {i} {k}")
        np.testing.assert_array_equal(got["actions"], golden[f"{variant}/out{i}/actions"])
        np.testing.assert_array_equal(got["rewards"][:, 0], golden[f"{variant}/out{i}/old_values"])
        # the single-store next observation of (t, e) is the observation of ((t + 1) % T, e)
        nxt = PC.sample_reference(stores, None, scalars, (j % T + 1) % T, j // T, T, None, img_range, tac_range)["observations"]
        for k in nxt:
            np.testing.assert_array_equal(got["next_observations"][k], nxt[k])


def test_ring_model_by_hand():
    """T = 3, 5 adds (k = 0..4): slots 0, 1, 2, 0, 1 are written in turn, so pos = 2 and the ring is full."""
    two = PC.RingModel(3)
    one = PC.RingModel(3, single_store=True)
    for m in (two, one):
        assert m.size() == 0 and m.valid_steps() == []
        m.add()
        m.add()
        assert (m.pos, m.full, m.size()) == (2, False, 2) and m.valid_steps() == [0, 1]
        for _ in range(3):
            m.add()
        assert (m.pos, m.full, m.size(), m.n_adds) == (2, True, 3, 5)
        assert m.step == [3, 4, 2]                            # slots 0 and 1 hold the overwriting adds, slot 2 the one add that went there
    assert two.obs == [("obs", 3), ("obs", 4), ("obs", 2)] and two.next_obs == [("next", 3), ("next", 4), ("next", 2)]
    assert two.valid_steps() == [0, 1, 2]
    assert [two.next_of(t) for t in range(3)] == [("next", 3), ("next", 4), ("next", 2)]
    # single store: add 4 wrote its observation to slot 1 and its next observation to slot 2 = pos, over the observation of add 2
    assert one.obs == [("obs", 3), ("obs", 4), ("next", 4)] and one.next_obs is None
    assert one.valid_steps() == [0, 1] and one.pos not in one.valid_steps()      # t = (u + pos) % T, u in [1, T)
    assert one.next_of(1) == ("next", 4)                      # the slot after the newest holds that step's next observation
    assert one.next_of(0) == ("obs", 4)                       # = the next observation of add 3, as the env returned it
    assert one.next_of(2) == ("obs", 3)                       # step pos: slot 2's scalars are add 2's, its 'next' would be add 3's observation
    # the last slot's next observation wraps to slot 0
    w = PC.RingModel(3, single_store=True)
    for _ in range(3):
        w.add()
    assert (w.pos, w.full) == (0, True) and w.obs == [("next", 2), ("obs", 1), ("obs", 2)]
    assert w.valid_steps() == [1, 2] and w.next_of(2) == ("next", 2)


def test_reward_normalisation_by_hand():
    # var + eps = 4 exactly in double: s = 2, so r / s is exact in float32; clip at 1.5
    got = PC.normalize_reward_reference([1.0, -2.5, 3.0, -3.0, 4.0, -8.0, 0.0], 4.0 - 1e-8, 1e-8, 1.5)
    assert got.dtype == np.float32
    np.testing.assert_array_equal(got, np.array([0.5, -1.25, 1.5, -1.5, 1.5, -1.5, 0.0], np.float32))
    # a scale float32 cannot represent: s = float32(sqrt(2 + 1e-8)), one rounding, then one IEEE division
    s32 = np.float32(math.sqrt(2.0 + 1e-8))
    got = PC.normalize_reward_reference([1.0, 3.0, -20.0], 2.0, 1e-8, 10.0)
    np.testing.assert_array_equal(got, np.array([np.float32(1.0) / s32, np.float32(3.0) / s32, -10.0], np.float32))
    exact = PC.normalize_reward_reference([1.0, 3.0, -20.0], 2.0, 1e-8, 10.0, dtype=np.float64)
    assert np.all(np.abs(got.astype(np.float64) - exact) <= 2.0 ** -22 * np.abs(exact))
    # the public helper reads the same numbers off a duck-typed env
    env = SimpleNamespace(norm_obs=False, norm_reward=True, ret_rms=SimpleNamespace(var=2.0), epsilon=1e-8, clip_reward=10.0)
    assert P.reward_normalization(env) == (float(s32), 10.0)
    assert P.reward_normalization(None) == (0.0, 0.0)
    assert P.reward_normalization(SimpleNamespace(norm_obs=False, norm_reward=False)) == (0.0, 0.0)
    with pytest.raises(ValueError, match="norm_obs"):
        P.reward_normalization(SimpleNamespace(norm_obs=True, norm_reward=True, ret_rms=SimpleNamespace(var=2.0), epsilon=1e-8, clip_reward=10.0))


SHAPES = {"image": (2, 8, 8, 3), "tactile": (2, 6, 4, 4)}
DTYPES = {"image": np.uint8, "tactile": np.float32}
REF_SHAPES = {"image": (4, 64, 64, 3), "tactile": (4, 6, 32, 32)}       # the reference's SAC observations: frame_stack 4, 2 sensors


def _buffer(**kw):
    args = dict(buffer_size=6, n_envs=2, obs_shapes=SHAPES, obs_dtypes=DTYPES, action_dim=3)
    args.update(kw)
    return m3l_amd.DeviceReplayBuffer(**args)


def test_constructor_touches_no_device_and_keeps_sb3_surface():
    buf = _buffer()
    assert (buf.buffer_size, buf.pos, buf.full, buf.size(), buf.frame_stack) == (3, 0, False, 0, 2)      # capacity in steps: 6 // 2
    assert (buf.optimize_memory_usage, buf.handle_timeout_termination) == (False, True)
    assert buf.obs_dtypes == {"image": torch.uint8, "tactile": torch.float32}
    assert _buffer(buffer_size=1, n_envs=2).buffer_size == 1                                             # max(1 // 2, 1)
    for name in ("reset", "add", "sample", "size", "store_bytes"):
        assert callable(getattr(buf, name))


def test_store_bytes_by_hand():
    """One transition of the reference's shapes: image 4 * 64 * 64 * 3 = 49152 elements, tactile 4 * 6 * 32 * 32 = 24576 elements."""
    n = 1000
    two = _buffer(buffer_size=n, n_envs=1, obs_shapes=REF_SHAPES, action_dim=7).store_bytes()
    assert two["observations"] == two["next_observations"] == n * (49152 + 4 * 24576) == n * 147456
    assert two["observations"] + two["next_observations"] == n * 294912
    assert two["scalars"] == n * 4 * (7 + 3) and two["total"] == n * 294912 + two["scalars"]
    one = _buffer(buffer_size=n, n_envs=1, obs_shapes=REF_SHAPES, obs_dtypes={"image": np.uint8, "tactile": np.uint8}, action_dim=7,
                  optimize_memory_usage=True, handle_timeout_termination=False).store_bytes()
    assert one["observations"] == n * 73728 and one["next_observations"] == 0
    assert one["scalars"] == n * 4 * (7 + 2) and one["total"] == n * 73728 + one["scalars"]
    # SB3's default of a million transitions in two stores: 295 GB
    big = _buffer(buffer_size=1_000_000, n_envs=1, obs_shapes=REF_SHAPES).store_bytes()
    assert big["observations"] + big["next_observations"] == 294_912_000_000
    # n_envs > 1: buffer_size // n_envs steps of n_envs rows
    assert _buffer(buffer_size=7, n_envs=2, obs_shapes=REF_SHAPES).store_bytes()["observations"] == 3 * 2 * 147456


def test_cpu_placement_is_refused():
    with pytest.raises(m3l_amd.M3LError, match="no CPU fallback"):
        _buffer(device="cpu")
    rows = torch.zeros(2, dtype=torch.int64)
    with pytest.raises(m3l_amd.M3LError, match="must live on the GPU"):
        P.gather_load(torch.zeros(3, 2, 1, 4, 4, 3), None, rows)
    with pytest.raises(m3l_amd.M3LError, match="must live on the GPU"):
        P.gather_rows(torch.zeros(3, 2, 1), torch.zeros(3, 2), torch.zeros(3, 2), None, rows)
    with pytest.raises(ValueError, match="neither an image nor a tactile store"):
        P.gather_load(None, None, rows)


@pytest.mark.parametrize("dt", [np.float64, np.int8, np.float16, torch.bfloat16, "int32"])
def test_observation_dtypes_other_than_uint8_and_float32_are_refused(dt):
    with pytest.raises(ValueError, match="uint8 or float32"):
        _buffer(obs_dtypes={"image": dt, "tactile": np.float32})
    with pytest.raises(ValueError, match="uint8 or float32"):
        _buffer(obs_dtypes={"image": np.uint8, "tactile": dt})


def test_other_constructor_rejections():
    with pytest.raises(ValueError, match="optimize_memory_usage=True needs handle_timeout_termination=False"):
        _buffer(optimize_memory_usage=True)
    assert _buffer(optimize_memory_usage=True, handle_timeout_termination=False).optimize_memory_usage
    for channels in (4, 7, 27, 0):
        with pytest.raises(ValueError, match=r"DeviceReplayBuffer: .*3 \* S"):
            _buffer(obs_shapes={"image": (2, 8, 8, 3), "tactile": (2, channels, 4, 4)})
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
    for kw in (dict(buffer_size=0), dict(n_envs=0), dict(action_dim=0)):
        with pytest.raises(ValueError, match="must be positive"):
            _buffer(**kw)


def test_add_and_sample_rejections():
    buf = _buffer()
    obs = {"image": np.zeros((2,) + SHAPES["image"], np.uint8), "tactile": np.zeros((2,) + SHAPES["tactile"], np.float32)}
    rest = (np.zeros((2, 3), np.float32), np.zeros(2, np.float32), np.zeros(2, bool), [{}, {}])
    with pytest.raises(ValueError, match="shape"):
        buf.add({"image": obs["image"][:1], "tactile": obs["tactile"]}, obs, *rest)
    with pytest.raises(ValueError, match=r"next_obs.*shape"):
        buf.add(obs, {"image": obs["image"], "tactile": obs["tactile"][:, :1]}, *rest)
    with pytest.raises(ValueError, match="observation keys"):
        buf.add({"image": obs["image"]}, obs, *rest)
    with pytest.raises(ValueError, match="observation keys"):
        buf.add(obs, {"tactile": obs["tactile"]}, *rest)
    with pytest.raises(ValueError, match="infos"):
        buf.add(obs, obs, *rest[:3], [{}])
    assert (buf.pos, buf.full) == (0, False) and buf.observations is None      # nothing was stored or allocated
    with pytest.raises(ValueError, match="empty"):
        buf.sample(4)
    with pytest.raises(ValueError, match="empty"):
        buf.sample(4, indices=([0], [0]))
    buf.pos = 2                                                # as after two add() calls (which need the GPU): steps 0 and 1 are valid
    with pytest.raises(ValueError, match="norm_obs"):
        buf.sample(4, env=SimpleNamespace(norm_obs=True, norm_reward=True))
    with pytest.raises(ValueError, match="batch_size"):
        buf.sample(0)
    for bad in (([0, 2], [0, 0]), ([-1], [0]), ([0], [2]), ([0], [-1]), ([], []), ([0, 1], [0]), ([[0]], [[0]]), ([0.5], [0]), [0, 1, 1], 3):
        with pytest.raises(ValueError, match="indices"):
            buf.sample(4, indices=bad)
    # a full single store: every step but pos
    one = _buffer(optimize_memory_usage=True, handle_timeout_termination=False)
    one.pos, one.full = 2, True
    assert one._valid_steps() == (0, 2) and one.size() == 3
    with pytest.raises(ValueError, match="indices"):
        one.sample(4, indices=([2], [0]))
    one.pos = 0
    assert one._valid_steps() == (1, 2)
    with pytest.raises(ValueError, match="indices"):
        one.sample(4, indices=([1, 0], [0, 0]))
    one.reset()
    assert (one.pos, one.full, one.size()) == (0, False, 0)


def _gather_load_rc(**kw):
    """m3l_replay_gather_load with arguments it must refuse before any launch (the pointers are never dereferenced on the host)."""
    a = dict(image=1 << 20, image_next=1 << 25, image_u8=0, H=8, W=8, img=(0.0, 1.0), image_out=1 << 21, image_next_out=1 << 26, tactile=1 << 22,
             tactile_next=None, tactile_u8=0, th=4, tw=4, S=2, tac=(-1.0, 1.0), T=3, n_envs=2, fs=2, rows=1 << 23, shift=0, B=4)
    a.update(kw)
    outs = (C.c_void_p * 16)(*([1 << 24] * 16))
    nouts = (C.c_void_p * 16)(*([1 << 27] * 16))
    return L.lib().m3l_replay_gather_load(a["image"], a["image_next"], a["image_u8"], a["H"], a["W"], a["img"][0], a["img"][1], a["image_out"],
                                          a["image_next_out"], a["tactile"], a["tactile_next"], a["tactile_u8"], a["th"], a["tw"], a["S"], a["tac"][0],
                                          a["tac"][1], outs, a.get("nouts", nouts), a["T"], a["n_envs"], a["fs"], a["rows"], a["shift"], a["B"], None)


@pytest.mark.parametrize("kw,msg", [
    (dict(S=0), "n_sensors=0"), (dict(S=9), "n_sensors=9"), (dict(img=(0.25, 0.25)), "empty image normalisation range"),
    (dict(tac=(1.0, 1.0)), "empty tactile normalisation range"), (dict(image=None, image_next=None, tactile=None), "neither an image nor a tactile store"),
    (dict(image=None), "a next store without its store"), (dict(B=0), "B=0"), (dict(T=0), "T=0"), (dict(H=0), "image H=0"), (dict(rows=None), "B=4"),
    (dict(image_next_out=None), "next-observation image output is NULL"), (dict(nouts=None), "next-observation tactile outputs are NULL"),
    (dict(shift=6), "row_shift=6"), (dict(shift=-1), "row_shift=-1"),
])
def test_entry_point_rejections_before_any_launch(kw, msg):
    assert _gather_load_rc(**kw) == 1
    assert msg in L.last_error() and "replay_gather_load" in L.last_error()


def test_rows_entry_point_refuses_bad_arguments():
    lib = L.lib()
    p = 1 << 20

    def rc(actions=p, rewards=p, dones=p, timeouts=p, T=3, n_envs=2, A=2, rows=p, shift=0, B=4, scale=0.0, clip=0.0, out=p):
        return lib.m3l_replay_gather_rows(actions, rewards, dones, timeouts, T, n_envs, A, rows, shift, B, scale, clip, out, out, out, None, None)
    for kw, msg in ((dict(A=0), "A=0"), (dict(B=0), "B=0"), (dict(T=0), "T=0"), (dict(rewards=None), "NULL"), (dict(actions=None), "NULL"),
                    (dict(out=None), "NULL"), (dict(rows=None), "NULL"), (dict(shift=6), "row_shift=6"), (dict(scale=-1.0), "reward_scale=-1"),
                    (dict(scale=float("inf")), "reward_scale=inf"), (dict(scale=2.0, clip=-1.0), "reward_clip=-1")):
        assert rc(**kw) == 1 and msg in L.last_error() and "replay_gather_rows" in L.last_error(), (kw, L.last_error())
