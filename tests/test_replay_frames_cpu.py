"""CPU-only checks of the frame-deduplicated replay store (m3l_amd/replay.py `frame_dedup=True`, csrc/replay.hip
m3l_replay_gather_load_frames): the restatements of tests/replay_frame_cases.py by hand and against the stacked observations of their own
streams, the memory arithmetic, and every rejection of the new surface.  No kernel is launched here: the C entry point is reached only with
arguments it refuses before any launch."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import m3l_amd
import replay_cases as PC
import replay_frame_cases as FC
import rollout_cases as RC
from m3l_amd import _lib as L
from m3l_amd import replay as P

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U8, F32 = np.uint8, np.float32
SHAPES = {"image": (2, 8, 8, 3), "tactile": (2, 6, 4, 4)}
DTYPES = {"image": U8, "tactile": F32}
REF_SHAPES = {"image": (4, 64, 64, 3), "tactile": (4, 6, 32, 32)}       # the reference's SAC observations: frame_stack 4, 2 sensors


def _buffer(**kw):
    args = dict(buffer_size=14, n_envs=2, obs_shapes=SHAPES, obs_dtypes=DTYPES, action_dim=3)
    args.update(kw)
    return m3l_amd.DeviceReplayBuffer(**args)


def test_exports_and_abi():
    assert L.lib().m3l_version() >= 413
    assert "m3l_replay_gather_load_frames" in L.EXPORTS and hasattr(L.lib(), "m3l_replay_gather_load_frames")
    hdr = open(os.path.join(ROOT, "include", "m3l_amd.h")).read()
    assert "int m3l_replay_gather_load_frames(" in hdr and "frame-deduplicated replay store (ABI 413)" in hdr
    assert callable(P.gather_load_frames)
    # the frame stores go through the stacked stores' validation, not a copy of it
    from m3l_amd import rollout as R
    assert P._check_stores is R._check_stores


def test_constructor_touches_no_device_with_the_new_keywords():
    buf = _buffer(frame_dedup=True, check_stacking=True)
    assert (buf.frame_dedup, buf.check_stacking, buf.buffer_size, buf.frame_stack, buf.pos, buf.full, buf.size()) == (True, True, 7, 2, 0, False, 0)
    assert buf.frames is None and buf.next_frames is None and buf.ages is None and buf.observations is None
    plain = _buffer()
    assert (plain.frame_dedup, plain.check_stacking) == (False, False)
    # nothing to deduplicate with one frame: accepted, the same code path
    one = _buffer(obs_shapes={"image": (1, 8, 8, 3)}, obs_dtypes={"image": U8}, frame_dedup=True)
    assert one.frame_stack == 1 and one.store_bytes()["observations"] == _buffer(obs_shapes={"image": (1, 8, 8, 3)},
                                                                                 obs_dtypes={"image": U8}).store_bytes()["observations"]


def test_new_constructor_rejections():
    with pytest.raises(ValueError, match=r"frame_dedup=True with frame_stack=2 needs a capacity of at least 3 steps"):
        _buffer(buffer_size=4, frame_dedup=True)                                  # 4 // 2 = 2 steps
    assert _buffer(buffer_size=6, frame_dedup=True).buffer_size == 3
    assert _buffer(buffer_size=4).buffer_size == 2                                # the stacked buffer keeps accepting it
    with pytest.raises(ValueError, match="at least 2 steps"):
        _buffer(buffer_size=2, obs_shapes={"image": (1, 8, 8, 3)}, obs_dtypes={"image": U8}, frame_dedup=True)
    with pytest.raises(ValueError, match="check_stacking=True checks the contract of frame_dedup=True"):
        _buffer(check_stacking=True)
    with pytest.raises(ValueError, match="optimize_memory_usage=True needs handle_timeout_termination=False"):
        _buffer(frame_dedup=True, optimize_memory_usage=True)


def test_store_bytes_by_hand():
    """One frame of the reference's shapes: image 64 * 64 * 3 = 12288 uint8, tactile 6 * 32 * 32 = 6144 float32 = 24576 B: 36864 B per step and
    store, against 147456 B stacked."""
    n = 1000
    kw = dict(buffer_size=n, n_envs=1, obs_shapes=REF_SHAPES, action_dim=7)
    two = _buffer(frame_dedup=True, **kw).store_bytes()
    assert two["observations"] == two["next_observations"] == n * (12288 + 24576) == n * 36864
    assert two["scalars"] == n * 4 * (7 + 3) + n * 4 and two["total"] == 2 * n * 36864 + two["scalars"]
    one = _buffer(frame_dedup=True, optimize_memory_usage=True, handle_timeout_termination=False, **kw).store_bytes()
    assert one["observations"] == n * 36864 and one["next_observations"] == 0
    assert one["scalars"] == n * 4 * (7 + 2) + n * 4 and one["total"] == n * 36864 + one["scalars"]
    stacked = _buffer(**kw).store_bytes()
    assert stacked["observations"] == 4 * two["observations"] and stacked["scalars"] == two["scalars"] - 4 * n
    # SB3's default of a million transitions
    big = dict(kw, buffer_size=1_000_000)
    assert _buffer(frame_dedup=True, **big).store_bytes()["total"] == 73_772_000_000 == 2 * 36864 * 10 ** 6 + 4 * 10 ** 6 * 10 + 4 * 10 ** 6
    assert _buffer(frame_dedup=True, optimize_memory_usage=True, handle_timeout_termination=False, **big).store_bytes()["total"] == \
        36_864_000_000 + 4 * 10 ** 6 * 9 + 4 * 10 ** 6
    # n_envs > 1: buffer_size // n_envs steps of n_envs frames
    assert _buffer(frame_dedup=True, buffer_size=15, n_envs=2, obs_shapes=REF_SHAPES).store_bytes()["observations"] == 7 * 2 * 36864


def _numbers(stack):
    """Frame numbers of a (fs, ...) stack of replay_frame_cases.make_frame's uint8 frames."""
    return [int(f.reshape(-1)[1]) for f in stack]


def test_stack_restatement_and_valid_steps_by_hand():
    """fs = 3, T = 5, one environment, episodes of 1, 2 and 4 steps.  Frames are numbered as the environment makes them: 0 the first reset
    frame, 1 the step of episode A, 2 the reset of episode B, 3 4 its steps, 5 the reset of C, 6 7 8 9 its steps, 10 the next reset, 11 a step."""
    fs, T = 3, 5
    st = FC.make_stream(8, 1, fs, (2, 2), (2, 2), 1, U8, U8, 2, seed=1, lengths=lambda fs_, e: [1, 2, 4])
    for key in ("image", "tactile"):
        assert [_numbers(st["obs"][key][k, 0]) for k in range(8)] == \
            [[0, 0, 0], [2, 2, 2], [2, 2, 3], [5, 5, 5], [5, 5, 6], [5, 6, 7], [6, 7, 8], [10, 10, 10]]
        assert [_numbers(st["next_obs"][key][k, 0]) for k in range(8)] == \
            [[0, 0, 1], [2, 2, 3], [2, 3, 4], [5, 5, 6], [5, 6, 7], [6, 7, 8], [7, 8, 9], [10, 10, 11]]
    assert st["ages"][:, 0].tolist() == [0, 0, 1, 0, 1, 2, 2, 0]                 # two consecutive 0s: the episode of one step
    assert st["dones"][:, 0].tolist() == [True, False, True, False, False, False, True, True]
    assert st["timeouts"][:, 0].tolist() == [True, False, False, False, False, False, True, False]      # truncated, terminated, truncated, terminated
    assert [bool(i.get("TimeLimit.truncated")) for (i,) in st["infos"]] == st["timeouts"][:, 0].tolist()
    assert _numbers(st["infos"][2][0]["terminal_observation"]["image"]) == [2, 3, 4]

    number = lambda tag: int((st["obs"] if tag[0] == "obs" else st["next_obs"])["image"][tag[1], 0, -1].reshape(-1)[1])      # noqa: E731
    # not full: every stored step, as the stacked buffer
    _, part = FC.fill_models(4, T, fs, False, st)
    assert part.valid_steps() == [0, 1, 2, 3] and part.ages[:4] == [[0], [0], [1], [0]] and part.ages[4] is None
    assert [number(x) for x in part.obs_frames(2, 0)] == [2, 2, 3] and [number(x) for x in part.next_frames(2, 0)] == [2, 3, 4]
    # 8 adds: slots 0 1 2 hold adds 5 6 7, slots 3 4 adds 3 4; pos = 3
    _, two = FC.fill_models(8, T, fs, False, st)
    assert (two.pos, two.full) == (3, True) and two.step == [5, 6, 7, 3, 4]
    assert two.valid_steps() == [0, 1, 2]                                          # T - (fs - 1) = 3 steps from pos + fs - 1 = 5 = slot 0
    assert two.obs_frames(0, 0) == [("obs", 3), ("obs", 4), ("obs", 5)] and two.next_frames(0, 0) == [("obs", 4), ("obs", 5), ("next", 5)]
    assert [[number(x) for x in two.obs_frames(t, 0)] for t in (0, 1, 2)] == [[5, 6, 7], [6, 7, 8], [10, 10, 10]]
    assert [[number(x) for x in two.next_frames(t, 0)] for t in (0, 1, 2)] == [[6, 7, 8], [7, 8, 9], [10, 10, 11]]
    # slot 4 = add 4 with age 1 is left out by the uniform rule although its one earlier frame survives; slot 3's neighbour is the newest step
    assert two.obs[(3 - 1) % T] == ("obs", 7)
    _, one = FC.fill_models(8, T, fs, True, st)
    assert one.obs[3] == ("next", 7) and one.valid_steps() == [1, 2]               # T - fs = 2 steps from pos + fs = 6 = slot 1
    assert [[number(x) for x in one.obs_frames(t, 0)] for t in (1, 2)] == [[6, 7, 8], [10, 10, 10]]
    # the single-store caveat: add 6 ended its episode; its next observation is the old episode's frames and the reset frame of the new one
    assert [number(x) for x in one.next_frames(1, 0)] == [7, 8, 10] and [number(x) for x in one.next_frames(2, 0)] == [10, 10, 11]
    # just full, pos = 0
    _, five = FC.fill_models(5, T, fs, False, st)
    assert (five.pos, five.full) == (0, True) and five.valid_steps() == [2, 3, 4]
    _, five1 = FC.fill_models(5, T, fs, True, st)
    assert five1.valid_steps() == [3, 4]
    # fs = 1: today's rules
    m1, f1 = FC.fill_models(8, T, 1, True, dict(ages=np.zeros((8, 1), int)))
    assert f1.valid_steps() == m1.valid_steps() == [4, 0, 1, 2]
    m2, f2 = FC.fill_models(8, T, 1, False, dict(ages=np.zeros((8, 1), int)))
    assert f2.valid_steps() == m2.valid_steps() == [0, 1, 2, 3, 4]


@pytest.mark.parametrize("single_store", [False, True], ids=["two_stores", "single_store"])
@pytest.mark.parametrize("fs", [1, 2, 3, 4])
def test_the_rule_rebuilds_the_streams_own_stacks(fs, single_store):
    """The streams of the GPU tests (T = 7, two environments): at every valid (t, e) the stacks put together from single frames by the restated
    rule are the stacked observations the environment produced; the buffer object's own (first, count) names the model's valid steps; and the
    stream holds every episode length the rule has to survive."""
    T, E = 7, 2
    st = FC.make_stream(17, E, fs, (8, 8), (4, 4), 2, U8, F32, 3, seed=10 + fs)
    for e in range(E):
        plan = FC.episode_lengths(fs, e)
        assert {1, 2, max(fs - 1, 1)} <= set(plan) and max(plan) >= fs + 2
    ends = [np.flatnonzero(st["dones"][:, e]).tolist() for e in range(E)]
    assert ends[0] != ends[1] and (st["dones"] & st["timeouts"]).any() and (st["dones"] & ~st["timeouts"]).any()
    assert any(st["ages"][k, e] == 0 and st["ages"][k + 1, e] == 0 for k in range(16) for e in range(E))
    buf = m3l_amd.DeviceReplayBuffer(T * E, E, {"image": (fs, 8, 8, 3), "tactile": (fs, 6, 4, 4)}, DTYPES, 3, optimize_memory_usage=single_store,
                                     handle_timeout_termination=not single_store, frame_dedup=True)
    for n_adds in (5, 7, 17):
        stacked, model = FC.fill_models(n_adds, T, fs, single_store, st)
        valid = model.valid_steps()
        assert set(valid) <= set(stacked.valid_steps()) and len(valid) == (n_adds if n_adds < T else T - (fs - 1) - int(single_store))
        buf.pos, buf.full = model.pos, model.full
        first, count = buf._valid_steps()
        assert [(first + u) % T for u in range(count)] == valid
        t = np.repeat(valid, E)
        e = np.tile(np.arange(E), len(valid))
        obs, nxt = FC.expected_from_model(model, st, t, e)
        k = np.array([model.step[x] for x in t])
        want = RC.vt_load_reference(RC.flatten_frame_stack({key: v[k, e] for key, v in st["obs"].items()}), fs)
        want_next = RC.vt_load_reference(RC.flatten_frame_stack({key: v[k, e] for key, v in st["next_obs"].items()}), fs)
        # the single store loses the terminal frame of a finished episode unless that step is the newest one
        keep = np.ones(len(t), bool) if not single_store else ~st["dones"][k, e] | (k == n_adds - 1)
        assert keep.any()
        for key in want:
            np.testing.assert_array_equal(obs[key], want[key])
            np.testing.assert_array_equal(nxt[key][keep], want_next[key][keep])
        # and the stacked restatement on the stacked stores says the same
        stores, nstores, scalars = FC.stacked_stores(stacked, st)
        ref = PC.sample_reference(stores, nstores, scalars, t, e, T)
        for key in want:
            np.testing.assert_array_equal(obs[key], ref["observations"][key])
            np.testing.assert_array_equal(nxt[key][keep], ref["next_observations"][key][keep])


def test_frames_reference_clamps_and_wraps():
    """frames_reference by hand: T = 3, one environment, fs = 3, frames whose first element is their slot."""
    frames = {"image": np.zeros((3, 1, 2, 2, 3), U8)}
    frames["image"][:, 0, 0, 0, 0] = [10, 20, 30]
    nxt = {"image": np.zeros((3, 1, 2, 2, 3), U8)}
    nxt["image"][:, 0, 0, 0, 0] = [11, 21, 31]
    first = lambda out: (out["image"][:, ::3, 0, 0] * 255).round().astype(int).tolist()      # noqa: E731  (B, fs): channel 0 of every frame
    obs, nob = FC.frames_reference(frames, nxt, np.array([[2], [0], [1]]), [0, 1, 2], 3, (0, 255))
    assert first(obs) == [[20, 30, 10], [20, 20, 20], [20, 20, 30]] and first(nob) == [[30, 10, 11], [20, 20, 21], [20, 30, 31]]
    obs2, nob2 = FC.frames_reference(frames, None, np.array([[100], [-3], [1]]), [0, 1, 2], 3, (0, 255))
    assert first(obs2) == first(obs) and first(nob2) == [[30, 10, 20], [20, 20, 30], [20, 30, 10]]


def test_valid_steps_and_injected_indices_on_the_host():
    buf = _buffer(frame_dedup=True)                               # T = 7, fs = 2
    buf.pos = 4
    assert buf._valid_steps() == (0, 4)
    buf.pos, buf.full = 3, True
    assert buf._valid_steps() == (4, 6)                           # every step but slot 3, the oldest
    for bad in (([3], [0]), ([4, 3], [0, 1]), ([7], [0]), ([4], [2])):
        with pytest.raises(ValueError, match="indices"):
            buf.sample(2, indices=bad)
    one = _buffer(frame_dedup=True, optimize_memory_usage=True, handle_timeout_termination=False)
    one.pos, one.full = 3, True
    assert one._valid_steps() == (5, 5)                           # not slot 3 (the newest next frame) nor slot 4 (its history is gone)
    for bad in (([3], [0]), ([4], [1]), ([5, 4], [0, 0])):
        with pytest.raises(ValueError, match="indices"):
            one.sample(2, indices=bad)
    one.reset()
    assert (one.pos, one.full, one.size()) == (0, False, 0) and one._episode_start.all()
    with pytest.raises(ValueError, match="empty"):
        one.sample(2)


def test_cpu_placement_and_missing_arguments_are_refused():
    rows = torch.zeros(2, dtype=torch.int64)
    ages = torch.zeros(3, 2, dtype=torch.int32)
    with pytest.raises(ValueError, match="neither an image nor a tactile frame store"):
        P.gather_load_frames(None, None, ages, rows, frame_stack=2)
    with pytest.raises(m3l_amd.M3LError, match="must live on the GPU"):
        P.gather_load_frames(torch.zeros(3, 2, 4, 4, 3), None, ages, rows, frame_stack=2)
    with pytest.raises(m3l_amd.M3LError, match="must live on the GPU"):
        P.gather_load_frames(None, torch.zeros(3, 2, 6, 4, 4), ages, rows, frame_stack=2)
    with pytest.raises(TypeError, match="frame_stack"):
        P.gather_load_frames(torch.zeros(3, 2, 4, 4, 3), None, ages, rows)
    with pytest.raises(m3l_amd.M3LError, match="no CPU fallback"):
        _buffer(frame_dedup=True, device="cpu")


def _frames_rc(**kw):
    """m3l_replay_gather_load_frames with arguments it must refuse before any launch (the pointers are never dereferenced on the host)."""
    a = dict(image=1 << 20, image_next=1 << 25, image_u8=0, H=8, W=8, img=(0.0, 1.0), image_out=1 << 21, image_next_out=1 << 26, tactile=1 << 22,
             tactile_next=None, tactile_u8=0, th=4, tw=4, S=2, tac=(-1.0, 1.0), ages=1 << 28, T=7, n_envs=2, fs=3, rows=1 << 23, shift=0, B=4)
    a.update(kw)
    outs = (C.c_void_p * 16)(*([1 << 24] * 16))
    nouts = (C.c_void_p * 16)(*([1 << 27] * 16))
    return L.lib().m3l_replay_gather_load_frames(
        a["image"], a["image_next"], a["image_u8"], a["H"], a["W"], a["img"][0], a["img"][1], a["image_out"], a["image_next_out"], a["tactile"],
        a["tactile_next"], a["tactile_u8"], a["th"], a["tw"], a["S"], a["tac"][0], a["tac"][1], a.get("outs", outs), a.get("nouts", nouts), a["ages"],
        a["T"], a["n_envs"], a["fs"], a["rows"], a["shift"], a["B"], None)


@pytest.mark.parametrize("kw,msg", [
    (dict(image=None, image_next=None, tactile=None), "neither an image nor a tactile frame store"), (dict(image=None), "a next store without its store"),
    (dict(tactile=None, tactile_next=1 << 29), "a next store without its store"), (dict(T=0), "T=0"), (dict(n_envs=0), "n_envs=0"),
    (dict(fs=0), "frame_stack=0"), (dict(B=0), "B=0"), (dict(rows=None), "B=4"), (dict(ages=None), "ages is NULL"), (dict(shift=14), "row_shift=14"),
    (dict(shift=-1), "row_shift=-1"), (dict(S=0), "n_sensors=0"), (dict(S=9), "n_sensors=9"), (dict(img=(0.25, 0.25)), "empty image normalisation range"),
    (dict(tac=(1.0, 1.0)), "empty tactile normalisation range"), (dict(H=0), "image H=0"), (dict(th=0), "tactile h=0"),
    (dict(image_out=None), "image H=8 W=8"), (dict(image_next_out=None), "next-observation image output is NULL"),
    (dict(nouts=None), "next-observation tactile outputs are NULL"), (dict(H=4096, W=4096, fs=600), "sample too large"),
])
def test_entry_point_rejections_before_any_launch(kw, msg):
    assert _frames_rc(**kw) == 1
    assert msg in L.last_error() and "replay_gather_load_frames" in L.last_error()
