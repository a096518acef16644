"""CPU-only checks of DeviceRolloutBuffer's random shift and frame store (m3l_rollout_gather_load_shift, m3l_rollout_gather_load_frames,
m3l_rollout_gather_load_frames_shift): the ABI, every rejection of the constructor, of `get(shifts=)` and of the functional forms — they happen
before any launch — the numpy restatement of the frame store against the streams' stacked observations, the slot rule's range over every int32
age, the coverage conditions of the streams and of the injected shifts, and the torch baseline of tools/rollout_feed_bench.py against the numpy
definition of the shift.  No kernel is launched here."""
import ctypes as C
import importlib.util
import os
import re

import numpy as np
import pytest
import torch

import m3l_amd
import rollout_aug_cases as RA
import shift_cases as SH
from m3l_amd import _lib as L
from m3l_amd import replay as P
from m3l_amd import rollout as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("m3l_rollout_gather_load_shift", "m3l_rollout_gather_load_frames", "m3l_rollout_gather_load_frames_shift")


# ---- the ABI
def _header():
    return open(os.path.join(ROOT, "include", "m3l_amd.h")).read()


def _declared(hdr, name):
    """The parameter list of `int name(...)` in the header, split at its commas."""
    m = re.search(r"\bint " + name + r"\(([^)]*)\)", hdr)
    assert m, name
    return [" ".join(p.split()) for p in m.group(1).split(",")]


def _ctype_of(param):
    if "*" in param:
        return C.c_void_p
    return {"int": C.c_int, "long": C.c_long, "float": C.c_float, "double": C.c_double}[param.split()[0]]


def test_exports_and_abi():
    assert L.lib().m3l_version() >= 418
    hdr = _header()
    assert "rollout augmentation and frame store (ABI 418)" in hdr and "parity unpinned" in hdr.split("(ABI 418)")[1]
    for name in NEW_SYMBOLS:
        assert name in L.EXPORTS and hasattr(L.lib(), name)
        res, args = L._SIGS[name]
        params = _declared(hdr, name)
        assert res is C.c_int and len(args) == len(params), (name, len(args), len(params))
        for a, p in zip(args, params):
            assert a is _ctype_of(p), (name, p, a)
    base = _declared(hdr, "m3l_rollout_gather_load")
    tail = ["const int32_t* shifts", "int image_pad", "int tactile_pad", "int B", "void* stream"]
    rename = lambda ps: [p.replace("_frames", "_store") for p in ps]      # noqa: E731
    # _shift: shifts and the two pads in front of B
    shift = _declared(hdr, "m3l_rollout_gather_load_shift")
    assert shift[:-5] == base[:-2] and shift[-5:] == tail
    # _frames: the frame stores in place of the stacked stores, ages in front of T
    frames = _declared(hdr, "m3l_rollout_gather_load_frames")
    i = base.index("int T")
    assert rename(frames) == base[:i] + ["const int32_t* ages"] + base[i:]
    assert "const void* image_frames" in frames and "const void* tactile_frames" in frames
    both = _declared(hdr, "m3l_rollout_gather_load_frames_shift")
    assert both[:-5] == frames[:-2] and both[-5:] == tail
    assert m3l_amd.RolloutBatch._fields == ("x", "actions", "old_values", "old_log_prob", "advantages", "returns")


def test_entry_points_refuse_bad_arguments_before_any_launch():
    lib = L.lib()
    p = 1 << 20
    outs = (C.c_void_p * 8)(*([1 << 24] * 8))
    head = (p, 0, 8, 8, 0.0, 1.0, p, p, 0, 4, 4, 2, -1.0, 1.0, outs)
    for pads, msg in (((-1, 0), "image_pad=-1"), ((0, 1 << 15), "tactile_pad=32768"), ((1 << 15, 0), "image_pad=32768")):
        assert lib.m3l_rollout_gather_load_shift(*head, 3, 2, 2, p, p, *pads, 4, None) == 1
        assert "rollout_gather_load_shift" in L.last_error() and msg in L.last_error(), L.last_error()
        assert lib.m3l_rollout_gather_load_frames_shift(*head, p, 3, 2, 2, p, p, *pads, 4, None) == 1
        assert "rollout_gather_load_frames_shift" in L.last_error() and msg in L.last_error(), L.last_error()
    assert lib.m3l_rollout_gather_load_frames(*head, None, 3, 2, 2, p, 4, None) == 1
    assert "rollout_gather_load_frames: ages is NULL" in L.last_error()
    assert lib.m3l_rollout_gather_load_frames_shift(*head, None, 3, 2, 2, p, p, 1, 1, 4, None) == 1
    assert "rollout_gather_load_frames_shift: ages is NULL" in L.last_error()
    # the error conditions of m3l_rollout_gather_load, under the new names
    none = (None,) + head[1:7] + (None,) + head[8:]
    assert lib.m3l_rollout_gather_load_shift(*none, 3, 2, 2, p, p, 1, 1, 4, None) == 1 and "neither an image nor a tactile store" in L.last_error()
    assert lib.m3l_rollout_gather_load_frames(*none, p, 3, 2, 2, p, 4, None) == 1 and "neither an image nor a tactile frame store" in L.last_error()
    assert lib.m3l_rollout_gather_load_shift(*head, 3, 2, 2, None, p, 1, 1, 4, None) == 1 and "rollout_gather_load_shift: T=3" in L.last_error()
    assert lib.m3l_rollout_gather_load_frames(*head, p, 0, 2, 2, p, 4, None) == 1 and "rollout_gather_load_frames: T=0" in L.last_error()
    empty = head[:4] + (1.0, 1.0) + head[6:]
    assert lib.m3l_rollout_gather_load_frames_shift(*empty, p, 3, 2, 2, p, p, 1, 1, 4, None) == 1 and "empty image normalisation range" in L.last_error()


# ---- the constructor, get(shifts=) and the functional forms
SHAPES = {"image": (2, 8, 12, 3), "tactile": (2, 6, 4, 8)}
DTYPES = {"image": np.uint8, "tactile": np.float32}


def _buffer(shapes=SHAPES, **kw):
    args = dict(buffer_size=5, n_envs=2, obs_shapes=shapes, obs_dtypes={k: DTYPES[k] for k in shapes}, action_dim=3)
    args.update(kw)
    return m3l_amd.DeviceRolloutBuffer(**args)


def test_constructor():
    b = _buffer()
    assert b.random_shift is None and b.last_shifts is None and b.frame_dedup is False and b.check_stacking is False
    assert b.observations is None and b.frames is None and b.ages is None
    assert _buffer(random_shift=None).random_shift is None
    assert _buffer(random_shift=4).random_shift == (4, 4)
    assert _buffer(random_shift=np.int64(3)).random_shift == (3, 3)
    assert _buffer(random_shift=dict(image=4, tactile=2)).random_shift == (4, 2)
    assert _buffer(random_shift=dict(image=4)).random_shift == (4, 0)          # a missing key means 0
    assert _buffer(random_shift=dict(tactile=1)).random_shift == (0, 1)
    assert _buffer(random_shift=(1 << 15) - 1).random_shift == ((1 << 15) - 1,) * 2
    for zero in (0, {}, dict(image=0), dict(image=0, tactile=0)):              # all-zero pads behave as None
        assert _buffer(random_shift=zero).random_shift is None
    assert _buffer(random_shift=2, frame_dedup=True, check_stacking=True).random_shift == (2, 2)
    for bad in (-1, 2.0, "3", True, [1, 2], 1.5):
        with pytest.raises(ValueError, match="DeviceRolloutBuffer: random_shift: the image and tactile pad .* must be an integer >= 0"):
            _buffer(random_shift=bad)
    for bad in (-1, 2.0, "3", True, None):
        with pytest.raises(ValueError, match="DeviceRolloutBuffer: random_shift: the tactile pad .* must be an integer >= 0"):
            _buffer(random_shift=dict(image=1, tactile=bad))
    for bad in (1 << 15, 1 << 40):
        with pytest.raises(ValueError, match=r"must be below 2\^15"):
            _buffer(random_shift=bad)
        with pytest.raises(ValueError, match=r"DeviceRolloutBuffer: random_shift: the image pad .* must be below 2\^15"):
            _buffer(random_shift=dict(image=bad))
    with pytest.raises(ValueError, match=r"DeviceRolloutBuffer: random_shift has the key\(s\) \['depth'\]; it takes 'image' and 'tactile'"):
        _buffer(random_shift=dict(image=1, depth=2))
    only_image = {"image": SHAPES["image"]}
    with pytest.raises(ValueError, match="a pad of 2 for 'tactile', which the buffer does not store"):
        _buffer(only_image, random_shift=dict(image=1, tactile=2))
    assert _buffer(only_image, random_shift=3).random_shift == (3, 0)          # one integer: every modality the buffer stores
    with pytest.raises(ValueError, match="DeviceRolloutBuffer: check_stacking=True checks the contract of frame_dedup=True and needs it"):
        _buffer(check_stacking=True)
    with pytest.raises(m3l_amd.M3LError, match="lives in GPU memory"):
        _buffer(device="cpu", frame_dedup=True)


def test_the_validation_is_shared_with_the_replay_buffer():
    """One copy of the pad / shift rules, in rollout.py; the replay buffer's messages are those of before."""
    for name in ("_check_pad", "_check_shifts", "_shift_pads", "_check_shift_pad", "_draw_shifts", "MAX_SHIFT_PAD"):
        assert getattr(P, name) is getattr(R, name), name
    assert not hasattr(m3l_amd.DeviceReplayBuffer, "_shift_pads")
    args = dict(buffer_size=14, n_envs=2, obs_shapes=SHAPES, obs_dtypes=DTYPES, action_dim=3)
    with pytest.raises(ValueError, match="DeviceReplayBuffer: random_shift: the image and tactile pad -1 must be an integer >= 0"):
        m3l_amd.DeviceReplayBuffer(random_shift=-1, **args)
    with pytest.raises(ValueError, match=r"DeviceReplayBuffer.sample: shifts must be a contiguous int32 tensor of shape \(B, 2, 2, 2\) = \(4, 2, 2, 2\): "
                                         r"\[sample, half, modality, \(dy, dx\)\]"):
        m3l_amd.DeviceReplayBuffer(random_shift=1, **args).sample(4, shifts=torch.zeros(4, 2, 2, dtype=torch.int32))


def test_store_bytes():
    """PPO's defaults: T = 4096, 8 environments, frame stack 4, image 64 x 64 x 3, 2 sensors at 32 x 32 x 3, float32 tactile."""
    shapes = {"image": (4, 64, 64, 3), "tactile": (4, 6, 32, 32)}
    img, tac = 64 * 64 * 3, 6 * 32 * 32
    for dt, isz in ((np.uint8, 1), (np.float32, 4)):
        mk = lambda **kw: m3l_amd.DeviceRolloutBuffer(4096, 8, shapes, {"image": dt, "tactile": np.float32}, 4, **kw)      # noqa: E731
        s, d = mk().store_bytes(), mk(frame_dedup=True).store_bytes()
        assert s["observations"] == 4096 * 8 * 4 * (img * isz + tac * 4) and s["scalars"] == 4 * 4096 * 8 * (4 + 6)
        assert d["observations"] == (4096 + 3) * 8 * (img * isz + tac * 4) and d["scalars"] == 4 * 4096 * 8 * (4 + 6 + 1)
        assert s["total"] == s["observations"] + s["scalars"] and d["total"] == d["observations"] + d["scalars"]
        assert set(s) == set(d) == {"observations", "scalars", "total"}
    assert round(s["observations"] / 1e9, 1) == 9.7 and round(d["observations"] / 1e9, 1) == 2.4


def test_get_refuses_wrong_shifts_before_any_launch():
    """The buffers are empty — no GPU here to fill them — and the shifts are refused first."""
    plain, buf = _buffer(), _buffer(random_shift=2)
    good = torch.zeros(4, 2, 2, dtype=torch.int32)
    idx = [0, 1, 2, 3]
    for b in (plain, _buffer(random_shift=0)):
        with pytest.raises(ValueError, match="DeviceRolloutBuffer.get: shifts= belongs to a buffer built with random_shift"):
            b.get(indices=idx, shifts=good)
    with pytest.raises(ValueError, match="DeviceRolloutBuffer.get: shifts= needs indices="):
        buf.get(batch_size=4, shifts=good)
    with pytest.raises(m3l_amd.M3LError, match="shifts must live on the GPU"):
        buf.get(indices=idx, shifts=good)
    for bad in (torch.zeros(3, 2, 2, dtype=torch.int32), torch.zeros(4, 2, 2, 2, dtype=torch.int32), torch.zeros(4, 2, 2, dtype=torch.int64),
                torch.zeros(4, 2, 4, dtype=torch.int32)[..., ::2], [[0, 0]], np.zeros((4, 2, 2), dtype=np.int32)):
        with pytest.raises(ValueError, match=r"shifts must be a contiguous int32 tensor of shape \(B, 2, 2\) = \(4, 2, 2\): \[sample, modality, "):
            buf.get(indices=idx, shifts=bad)
    with pytest.raises(ValueError, match=r"= \(3, 2, 2\)"):
        buf.get(indices=[0, 1, 2], shifts=good)
    # without shifts the first complaint is the one of before
    with pytest.raises(ValueError, match="the buffer is not full"):
        buf.get(indices=idx)


def test_functional_forms_refuse_bad_arguments_before_any_launch():
    i64 = torch.zeros(2, dtype=torch.int64)
    s32 = torch.zeros(2, 2, 2, dtype=torch.int32)
    with pytest.raises(m3l_amd.M3LError, match="gather_load: image_store must live on the GPU"):
        R.gather_load(torch.zeros(3, 2, 1, 4, 4, 3), None, i64, shifts=s32, shift_pad=(1, 0))
    with pytest.raises(m3l_amd.M3LError, match="gather_load_frames: image_frames must live on the GPU"):
        R.gather_load_frames(torch.zeros(3, 2, 4, 4, 3), None, torch.zeros(3, 2, dtype=torch.int32), i64, 1)
    with pytest.raises(ValueError, match="gather_load_frames: neither an image nor a tactile frame store"):
        R.gather_load_frames(None, None, torch.zeros(3, 2, dtype=torch.int32), i64, 1)
    with pytest.raises(ValueError, match="gather_load: neither an image nor a tactile store"):
        R.gather_load(None, None, i64, shifts=s32, shift_pad=(1, 1))
    # what can be told without a device tensor: a monkeypatched _require_cuda lets the shape / dtype checks be reached on CPU tensors
    mp = pytest.MonkeyPatch()
    mp.setattr(R, "_require_cuda", lambda t, what: None)
    try:
        img5, img6 = torch.zeros(4, 2, 4, 4, 3), torch.zeros(3, 2, 2, 4, 4, 3)
        ages = torch.zeros(3, 2, dtype=torch.int32)
        for bad_idx in (torch.zeros(2, dtype=torch.int32), torch.zeros(2, 1, dtype=torch.int64), torch.zeros(4, dtype=torch.int64)[::2]):
            with pytest.raises(ValueError, match="gather_load_frames: idx must be a contiguous 1-D int64 tensor"):
                R.gather_load_frames(img5, None, ages, bad_idx, 2)
        with pytest.raises(ValueError, match=r"gather_load_frames: image_frames must be a contiguous uint8 / float32 \(T, n_envs, ...\) tensor of 5"):
            R.gather_load_frames(img6, None, ages, i64, 2)
        with pytest.raises(ValueError, match="gather_load_frames: image_frames must be a contiguous"):
            R.gather_load_frames(img5.double(), None, ages, i64, 2)
        with pytest.raises(ValueError, match="gather_load_frames: image_frames has 4 channels"):
            R.gather_load_frames(torch.zeros(4, 2, 4, 4, 4), None, ages, i64, 2)
        with pytest.raises(ValueError, match="gather_load_frames: frame_stack=0"):
            R.gather_load_frames(img5, None, ages, i64, 0)
        with pytest.raises(ValueError, match=r"frame stores of 4 slots hold no step at frame_stack=5"):
            R.gather_load_frames(img5, None, ages, i64, 5)
        for bad_ages in (None, torch.zeros(4, 2, dtype=torch.int32), torch.zeros(3, 2, dtype=torch.int64), torch.zeros(3, 4, dtype=torch.int32)[:, ::2]):
            with pytest.raises(ValueError, match=r"gather_load_frames: ages must be a contiguous int32 tensor of shape \(T, n_envs\) = \(3, 2\)"):
                R.gather_load_frames(img5, None, bad_ages, i64, 2)
        for fn, args in ((R.gather_load, (img6, None, i64)), (R.gather_load_frames, (img5, None, ages, i64, 2))):
            who = fn.__name__
            with pytest.raises(ValueError, match=who + r": shift_pad must be a pair \(image_pad, tactile_pad\)"):
                fn(*args, shifts=s32, shift_pad=3)
            with pytest.raises(ValueError, match=who + ": the image pad -1 must be an integer >= 0"):
                fn(*args, shifts=s32, shift_pad=(-1, 0))
            with pytest.raises(ValueError, match=who + r": the tactile pad 32768 must be below 2\^15"):
                fn(*args, shift_pad=(0, 1 << 15))
            for bad in (torch.zeros(2, 2, 2, 2, dtype=torch.int32), torch.zeros(3, 2, 2, dtype=torch.int32), torch.zeros(2, 2, 2, dtype=torch.int64)):
                with pytest.raises(ValueError, match=who + r": shifts must be a contiguous int32 tensor of shape \(B, 2, 2\) = \(2, 2, 2\)"):
                    fn(*args, shifts=bad, shift_pad=(1, 0))
    finally:
        mp.undo()


def test_add_refuses_a_wrong_observation_before_any_allocation():
    buf = _buffer(frame_dedup=True)
    z = np.zeros(2, np.float32)
    with pytest.raises(ValueError, match=r"DeviceRolloutBuffer.add: observation 'image' has shape"):
        buf.add({"image": np.zeros((2, 3, 8, 12, 3), np.uint8), "tactile": np.zeros((2,) + SHAPES["tactile"], np.float32)}, np.zeros((2, 3)), z, z, z, z)
    assert buf.frames is None and buf.pos == 0


# ---- the restatements
@pytest.mark.parametrize("name", sorted(RA.CONFIGS))
def test_frame_store_restatement_rebuilds_the_stacked_stores(name):
    """Both rollouts of every stream, every (t, e, k): the frames that add() stores, read through the slot rule, are the stacked observations."""
    for T in RA.ROLLOUT_T:
        ro = RA.make_rollouts(name, T, seed=3)
        fs = ro["fs"]
        for r in (0, 1):
            sl = RA.rollout_slice(ro, r)
            for key in ("image", "tactile"):
                obs = ro["obs"][key][sl]
                frames, ages = RA.frame_store_reference(obs, ro["episode_start"][sl], fs)
                assert frames.shape == (T + fs - 1, RA.E) + obs.shape[3:] and ages.shape == (T, RA.E) and ages.dtype == np.int32
                assert np.array_equal(RA.stacked_from_frames(frames, ages, fs), obs), (name, T, r, key)
                # the ages are the true ages clamped, but at the rollout's first step, where the prologue holds the real stack
                want = np.minimum(ro["true_age"][sl], fs - 1)
                want[0] = np.where(ro["episode_start"][sl][0], 0, fs - 1)
                assert np.array_equal(ages, want), (name, T, r)
        # the streams keep the contract add() relies on: rolling stacks, a constant stack at an episode's first step
        for key in ("image", "tactile"):
            o = ro["obs"][key]
            for k in range(2 * T):
                for e in range(RA.E):
                    if ro["episode_start"][k, e]:
                        assert all(np.array_equal(o[k, e, j], o[k, e, 0]) for j in range(fs))
                    else:
                        assert np.array_equal(o[k, e, :-1], o[k - 1, e, 1:])


def test_slot_rule_stays_inside_its_window_for_every_age():
    ages = [SH.INT32_MIN, SH.INT32_MIN + 1, -2 ** 20, -1, 0, 1, 2, 3, 4, 5, 2 ** 20, SH.INT32_MAX - 1, SH.INT32_MAX]
    for fs in (1, 2, 3, 4):
        for t in (0, 1, 6, 4095):
            for age in ages:
                slots = [RA.frame_slot(t, k, fs, age) for k in range(fs)]
                assert all(t <= s <= t + fs - 1 for s in slots), (fs, t, age, slots)
                assert slots[-1] == t + fs - 1 and slots == sorted(slots)          # the newest frame is the step's own; older frames lie before
                assert slots == [RA.frame_slot(t, k, fs, min(max(age, 0), fs - 1)) for k in range(fs)]
            assert [RA.frame_slot(t, k, fs, 0) for k in range(fs)] == [t + fs - 1] * fs          # an episode's first step: one frame fs times
            assert [RA.frame_slot(t, k, fs, fs - 1) for k in range(fs)] == list(range(t, t + fs))
    assert [RA.frame_slot(5, k, 4, 1) for k in range(4)] == [7, 7, 7, 8]          # written out: reach 1 at fs = 4
    assert [RA.frame_slot(5, k, 4, 2) for k in range(4)] == [6, 6, 7, 8]
    assert RA.next_ages([0, 1, 2, 2], [False, False, False, True], 3, False).tolist() == [1, 2, 2, 0]
    assert RA.next_ages(None, [False, True], 3, True).tolist() == [2, 0]


def test_the_second_rollouts_cover_every_kind_of_start():
    assert RA.coverage_missing(3) == []
    name = next(n for n in sorted(RA.CONFIGS) if RA.CONFIGS[n][0] == 3)
    ro5, ro7 = RA.make_rollouts(name, 5, 0), RA.make_rollouts(name, 7, 0)
    # the starts named in the cases' docstring: step 5 meets environment 0 at an episode start and environment 1 three steps into an episode,
    # step 7 meets environment 0 one step into an episode and environment 1 at a start
    assert ro5["episode_start"][5].tolist() == [True, False] and ro5["true_age"][5, 1] == 3
    assert ro7["episode_start"][7].tolist() == [False, True] and ro7["true_age"][7, 0] == 1
    assert ro5["episode_start"][0].all() and ro5["dones"].shape == (2, RA.E)


@pytest.mark.parametrize("name", sorted(RA.CONFIGS))
def test_the_injected_shifts_cover_every_case(name):
    fs, image_hw, tactile_hw, S, dtypes, pads = RA.CONFIGS[name]
    shifts = RA.injected_shifts(pads)
    assert shifts.dtype == np.int32 and shifts.shape[1:] == (2, 2) and shifts.flags["C_CONTIGUOUS"]
    assert shifts.shape[0] > 3 * max(RA.ROLLOUT_T) * RA.E          # every flat index meets several shifts
    for m, (pad, W) in enumerate(zip(pads, (image_hw[1], tactile_hw[1]))):
        if pad:
            assert SH.covers(shifts[:, None], m, pad, W) == [], (name, m)
            have = {tuple(v) for v in SH.clamp_shift(shifts[:, m], pad).tolist()}
            assert have == {(dy, dx) for dy in range(-pad, pad + 1) for dx in range(-pad, pad + 1)}, (name, m)


def _bench_module():
    spec = importlib.util.spec_from_file_location("rollout_feed_bench", os.path.join(ROOT, "tools", "rollout_feed_bench.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.mark.parametrize("name", sorted(RA.CONFIGS))
def test_the_benchmarks_torch_baseline_is_the_numpy_definition(name):
    """tools/rollout_feed_bench.py --shift compares the shifted launch with torch ops; an index of theirs that leaves the tensor would be read by
    torch.gather unchecked on a device, so the function is held to the definition here, on CPU tensors, with the injected shifts' out-of-range
    and INT32-end entries."""
    baseline = _bench_module().torch_shift_baseline
    fs, image_hw, tactile_hw, S, dtypes, pads = RA.CONFIGS[name]
    shifts = RA.injected_shifts(pads)
    B = shifts.shape[0]
    g = np.random.default_rng(5)
    for m, (hw, pad) in enumerate(zip((image_hw, tactile_hw), pads)):
        x = g.random((B, 3 * fs) + tuple(hw), dtype=np.float32)
        got = baseline(torch.from_numpy(x), torch.from_numpy(shifts[:, m]), pad)
        assert got.dtype == torch.float32 and np.array_equal(got.numpy(), SH.random_shift_reference(x, shifts[:, m], pad)), (name, m)
