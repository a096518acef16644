"""CPU-only checks of the random-shift augmentation (DeviceReplayBuffer(random_shift=), m3l_replay_gather_load_shift,
m3l_replay_gather_load_frames_shift): the restatement of tests/shift_cases.py against torch's replicate padding for every shift of the range
and against an example written out by hand, the clamp, the ABI, the rejections of the constructor and of `sample(shifts=)` — they happen before
any launch — and the coverage condition of the shifts that test_replay_shift_gpu.py injects.  No kernel is launched here."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import m3l_amd
import shift_cases as SH
from m3l_amd import _lib as L
from m3l_amd import replay as P

NEW_SYMBOLS = ("m3l_replay_gather_load_shift", "m3l_replay_gather_load_frames_shift")


def _ramp(shape):
    """Non-integer float32 values, every element distinct."""
    return (np.arange(int(np.prod(shape)), dtype=np.float32) * np.float32(1.25) + np.float32(0.5)).reshape(shape)


@pytest.mark.parametrize("H,W,p", [(5, 7, 3), (3, 4, 4)])
def test_restatement_is_replicate_pad_and_crop_for_every_shift(H, W, p):
    """(3, 4) at p = 4: the pad is at least W, a whole row can leave the frame."""
    x = _ramp((2, 3, H, W))
    padded = F.pad(torch.from_numpy(x), (p, p, p, p), mode="replicate").numpy()
    for dy in range(-p, p + 1):
        for dx in range(-p, p + 1):
            want = padded[..., p + dy:p + dy + H, p + dx:p + dx + W]
            got = SH.random_shift_reference(x, [(dy, dx), (dy, dx)], p)
            assert got.dtype == x.dtype and np.array_equal(got, want), (dy, dx)
    # one shift per sample: sample 0 and sample 1 through different shifts in one call
    got = SH.random_shift_reference(x, [(p, -p), (-1, 2)], p)
    assert np.array_equal(got[0], padded[0, :, 2 * p:2 * p + H, 0:W]) and np.array_equal(got[1], padded[1, :, p - 1:p - 1 + H, p + 2:p + 2 + W])


def test_restatement_against_an_example_written_out_by_hand():
    x = np.array([[1, 2, 3], [4, 5, 6], [7, 8, 9]], dtype=np.float32).reshape(1, 1, 3, 3)
    by_hand = {(0, 0): [[1, 2, 3], [4, 5, 6], [7, 8, 9]],
               (1, 0): [[4, 5, 6], [7, 8, 9], [7, 8, 9]],             # dy = 1: every output row reads the row below; the last repeats
               (0, -1): [[1, 1, 2], [4, 4, 5], [7, 7, 8]],            # dx = -1: every output pixel reads its left neighbour; the first repeats
               (-1, 1): [[2, 3, 3], [2, 3, 3], [5, 6, 6]],
               (2, 2): [[9, 9, 9], [9, 9, 9], [9, 9, 9]],
               (-2, 1): [[2, 3, 3], [2, 3, 3], [2, 3, 3]]}
    for s, want in by_hand.items():
        assert SH.random_shift_reference(x, [s], 2)[0, 0].tolist() == want, s


def test_zero_shift_is_the_identity_and_out_of_range_shifts_are_clamped():
    x = _ramp((3, 2, 5, 7))
    assert np.array_equal(SH.random_shift_reference(x, np.zeros((3, 2), dtype=np.int32), 3), x)
    assert np.array_equal(SH.random_shift_reference(x, [(3, -3), (1, 1), (-2, 0)], 0), x)          # a pad of 0 clamps every shift to nothing
    for big in (1000, SH.INT32_MAX, -1000, SH.INT32_MIN):
        sign = 1 if big > 0 else -1
        for p in (1, 3):
            got = SH.random_shift_reference(x, np.array([(big, -big if big != SH.INT32_MIN else SH.INT32_MAX)] * 3, dtype=np.int64), p)
            assert np.array_equal(got, SH.random_shift_reference(x, [(sign * p, -sign * p)] * 3, p)), (big, p)
    assert SH.clamp_shift(np.array([SH.INT32_MIN, -4, -3, 0, 3, 4, SH.INT32_MAX], dtype=np.int32), 3).tolist() == [-3, -3, -3, 0, 3, 3, 3]
    assert SH.clamp_shift([5, -5], 0).tolist() == [0, 0]


# ---- the ABI
def _header():
    return open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "m3l_amd.h")).read()


def _declared(hdr, name):
    """The parameter list of `int name(...)` in the header, split at its commas."""
    m = re.search(r"\bint " + name + r"\(([^)]*)\)", hdr)
    assert m, name
    return [" ".join(p.split()) for p in m.group(1).split(",")]


def _ctype_of(param):
    if "*" in param:
        return (C.c_void_p,)
    return {"int": (C.c_int,), "long": (C.c_long,), "float": (C.c_float,), "double": (C.c_double,)}[param.split()[0]]


def test_exports_and_abi():
    assert L.lib().m3l_version() >= 417
    hdr = _header()
    assert "random-shift augmentation (ABI 417)" in hdr
    for name in NEW_SYMBOLS:
        assert name in L.EXPORTS and hasattr(L.lib(), name)
        res, args = L._SIGS[name]
        params = _declared(hdr, name)
        assert res is C.c_int and len(args) == len(params), (name, len(args), len(params))
        for a, p in zip(args, params):
            assert a in _ctype_of(p), (name, p, a)
    # each new entry is its _rows2 neighbour with shifts and the two pads in front of B
    for two, new in (("m3l_replay_gather_load_rows2", "m3l_replay_gather_load_shift"),
                     ("m3l_replay_gather_load_frames_rows2", "m3l_replay_gather_load_frames_shift")):
        a, b = _declared(hdr, two), _declared(hdr, new)
        assert b[:-5] == a[:-2] and b[-5:] == ["const int32_t* shifts", "int image_pad", "int tactile_pad", "int B", "void* stream"], new
    # the batch types are as they were
    assert m3l_amd.ReplayBatch._fields == ("observations", "actions", "next_observations", "dones", "rewards", "rows")
    assert m3l_amd.NStepReplayBatch._fields == m3l_amd.ReplayBatch._fields + ("discounts", "next_rows")
    assert m3l_amd.PrioritizedReplayBatch._fields == m3l_amd.NStepReplayBatch._fields + ("weights",)


def test_entry_points_refuse_bad_arguments_before_any_launch():
    lib = L.lib()
    p = 1 << 20
    outs = (C.c_void_p * 16)(*([1 << 24] * 16))
    head = (p, p, 0, 8, 8, 0.0, 1.0, p, p, p, p, 0, 4, 4, 2, -1.0, 1.0, outs, outs)
    for pads, msg in (((-1, 0), "image_pad=-1"), ((0, 1 << 15), "tactile_pad=32768"), ((1 << 15, 0), "image_pad=32768")):
        assert lib.m3l_replay_gather_load_shift(*head, 3, 2, 2, p, 0, None, p, *pads, 4, None) == 1
        assert "replay_gather_load_shift" in L.last_error() and msg in L.last_error(), L.last_error()
        assert lib.m3l_replay_gather_load_frames_shift(*head, p, 3, 2, 2, p, 0, None, p, *pads, 4, None) == 1
        assert "replay_gather_load_frames_shift" in L.last_error() and msg in L.last_error(), L.last_error()
    assert lib.m3l_replay_gather_load_frames_shift(*head, None, 3, 2, 2, p, 0, None, p, 1, 1, 4, None) == 1
    assert "replay_gather_load_frames_shift: ages is NULL" in L.last_error()
    assert lib.m3l_replay_gather_load_shift(*head, 3, 2, 2, p, 6, None, p, 1, 1, 4, None) == 1
    assert "replay_gather_load_shift: row_shift=6" in L.last_error()
    assert lib.m3l_replay_gather_load_shift(*head, 3, 2, 2, None, 0, None, p, 1, 1, 4, None) == 1 and "replay_gather_load_shift" in L.last_error()


# ---- the constructor and sample(shifts=)
SHAPES = {"image": (2, 8, 12, 3), "tactile": (2, 6, 4, 8)}
DTYPES = {"image": np.uint8, "tactile": np.float32}


def _buffer(shapes=SHAPES, **kw):
    args = dict(buffer_size=14, n_envs=2, obs_shapes=shapes, obs_dtypes={k: DTYPES[k] for k in shapes}, action_dim=3)
    args.update(kw)
    return m3l_amd.DeviceReplayBuffer(**args)


def test_constructor():
    assert _buffer().random_shift is None and _buffer().last_shifts is None
    assert _buffer(random_shift=None).random_shift is None
    assert _buffer(random_shift=4).random_shift == (4, 4)
    assert _buffer(random_shift=np.int64(3)).random_shift == (3, 3)
    assert _buffer(random_shift=dict(image=4, tactile=2)).random_shift == (4, 2)
    assert _buffer(random_shift=dict(image=4)).random_shift == (4, 0)          # a missing key means 0
    assert _buffer(random_shift=dict(tactile=1)).random_shift == (0, 1)
    assert _buffer(random_shift=(1 << 15) - 1).random_shift == ((1 << 15) - 1,) * 2
    # all-zero pads behave as None
    for zero in (0, {}, dict(image=0), dict(image=0, tactile=0)):
        assert _buffer(random_shift=zero).random_shift is None
    # with every mode the buffer has
    for kw in (dict(frame_dedup=True), dict(n_steps=3), dict(prioritized=True), dict(optimize_memory_usage=True, handle_timeout_termination=False),
               dict(frame_dedup=True, n_steps=2, prioritized=True)):
        assert _buffer(random_shift=2, **kw).random_shift == (2, 2)
    for bad in (-1, 2.0, "3", True, [1, 2], 1.5):
        with pytest.raises(ValueError, match="random_shift: the image and tactile pad .* must be an integer >= 0"):
            _buffer(random_shift=bad)
    for bad in (-1, 2.0, "3", True, None):
        with pytest.raises(ValueError, match="random_shift: the tactile pad .* must be an integer >= 0"):
            _buffer(random_shift=dict(image=1, tactile=bad))
    for bad in (1 << 15, 1 << 40):
        with pytest.raises(ValueError, match=r"must be below 2\^15"):
            _buffer(random_shift=bad)
        with pytest.raises(ValueError, match=r"random_shift: the image pad .* must be below 2\^15"):
            _buffer(random_shift=dict(image=bad))
    with pytest.raises(ValueError, match=r"random_shift has the key\(s\) \['depth'\]; it takes 'image' and 'tactile'"):
        _buffer(random_shift=dict(image=1, depth=2))
    only_image = {"image": SHAPES["image"]}
    with pytest.raises(ValueError, match="a pad of 2 for 'tactile', which the buffer does not store"):
        _buffer(only_image, random_shift=dict(image=1, tactile=2))
    assert _buffer(only_image, random_shift=dict(image=1, tactile=0)).random_shift == (1, 0)
    assert _buffer(only_image, random_shift=3).random_shift == (3, 0)          # one integer: every modality the buffer stores


def test_sample_refuses_wrong_shifts_before_any_launch():
    """The buffers are empty — no GPU here to fill them — and the shifts are refused first."""
    plain, buf = _buffer(), _buffer(random_shift=2)
    good = torch.zeros(4, 2, 2, 2, dtype=torch.int32)
    with pytest.raises(ValueError, match="shifts= belongs to a buffer built with random_shift"):
        plain.sample(4, shifts=good)
    with pytest.raises(ValueError, match="shifts= belongs to a buffer built with random_shift"):
        _buffer(random_shift=0).sample(4, shifts=good)
    # every tensor on the CPU is refused as the other arguments are
    with pytest.raises(m3l_amd.M3LError, match="shifts must live on the GPU"):
        buf.sample(4, shifts=good)
    # shape, dtype and contiguity are looked at first, wherever the tensor lies
    for bad in (torch.zeros(3, 2, 2, 2, dtype=torch.int32), torch.zeros(4, 2, 2, dtype=torch.int32), torch.zeros(4, 2, 2, 2, dtype=torch.int64),
                torch.zeros(4, 2, 2, 4, dtype=torch.int32)[..., ::2], [[0, 0]], np.zeros((4, 2, 2, 2), dtype=np.int32)):
        with pytest.raises(ValueError, match=r"shifts must be a contiguous int32 tensor of shape \(B, 2, 2, 2\) = \(4, 2, 2, 2\)"):
            buf.sample(4, shifts=bad)
    # B is the number of indices where there are any
    with pytest.raises(ValueError, match=r"= \(3, 2, 2, 2\)"):
        buf.sample(4, indices=([0, 1, 2], [0, 0, 0]), shifts=good)
    with pytest.raises(m3l_amd.M3LError, match="must live on the GPU"):
        P.gather_load(torch.zeros(3, 2, 1, 4, 4, 3), None, torch.zeros(2, dtype=torch.int64), shifts=torch.zeros(2, 2, 2, 2, dtype=torch.int32),
                      shift_pad=(1, 0))


# ---- the coverage condition of the shifts the GPU test injects
@pytest.mark.parametrize("name", sorted(SH.CONFIGS))
def test_the_injected_shifts_cover_every_case(name):
    fs, image_hw, tactile_hw, S, dtypes, pads = SH.CONFIGS[name]
    shifts = SH.injected_shifts(pads)
    assert shifts.dtype == np.int32 and shifts.shape[1:] == (2, 2, 2)
    for m, (pad, W) in enumerate(zip(pads, (image_hw[1], tactile_hw[1]))):
        if pad:
            assert SH.covers(shifts, m, pad, W) == [], (name, m)
            for half in (0, 1):         # each half on its own sees every shift of the range
                have = {tuple(v) for v in SH.clamp_shift(shifts[:, half, m], pad).tolist()}
                assert have == {(dy, dx) for dy in range(-pad, pad + 1) for dx in range(-pad, pad + 1)}, (name, m, half)
    assert (shifts[:, 0] != shifts[:, 1]).any(axis=(1, 2)).sum() > shifts.shape[0] // 2          # the halves of most samples differ
    # the condition is one: a list without the corners, the odd dx or the out-of-range entries misses it
    assert SH.covers(np.zeros((4, 2, 2, 2), dtype=np.int32), 0, 3, 12) != []
    assert "an entry above the range" in SH.covers(np.clip(shifts, -pads[0], pads[0]), 0, pads[0], image_hw[1])


def test_the_streams_differ_in_every_neighbour_and_keep_the_stacking_contract():
    for name, (fs, image_hw, tactile_hw, S, dtypes, pads) in SH.CONFIGS.items():
        st = SH.make_stream(fs, image_hw, tactile_hw, S, dtypes[0], dtypes[1], seed=1)
        img, tac = st["obs"]["image"], st["obs"]["tactile"]
        assert img.shape == (SH.N_ADDS, SH.E, fs) + image_hw + (3,) and tac.shape == (SH.N_ADDS, SH.E, fs, 3 * S) + tactile_hw
        assert img.dtype == dtypes[0] and tac.dtype == dtypes[1]
        f = img[3, 0, -1]
        assert (f[:, 1:] != f[:, :-1]).all() and (f[1:] != f[:-1]).all() and (f[..., 1:] != f[..., :-1]).all(), name      # pixels, rows, channels
        g = tac[3, 1, -1]
        assert (g[:, :, 1:] != g[:, :, :-1]).all() and (g[:, 1:] != g[:, :-1]).all() and (g[1:] != g[:-1]).all(), name      # and planes / sensors
        assert (img[3, 0, -1] != img[3, 1, -1]).all() and (img[3, 0, -1] != img[4, 0, -1]).all(), name                    # environments, steps
        if np.dtype(dtypes[0]) == np.float32:
            assert (img != np.round(img)).all()
        # the contract of frame_dedup: rolling stacks, a constant stack at an episode's first step, obs = the previous next_obs otherwise
        for k in ("image", "tactile"):
            o, n = st["obs"][k], st["next_obs"][k]
            assert np.array_equal(n[:, :, :-1], o[:, :, 1:])
            for e in range(SH.E):
                for step in range(SH.N_ADDS):
                    if step == 0 or st["dones"][step - 1, e]:
                        assert all(np.array_equal(o[step, e, j], o[step, e, 0]) for j in range(fs))
                    else:
                        assert np.array_equal(o[step, e], n[step - 1, e])
        assert st["dones"].any(axis=0).all() and any(i["TimeLimit.truncated"] for row in st["infos"] for i in row)
