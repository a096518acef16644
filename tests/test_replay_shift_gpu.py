"""The random-shift augmentation of the device-resident replay buffer on a real MI355X (m3l_amd/replay.py `random_shift=`, csrc/replay.hip
m3l_replay_gather_load_shift / m3l_replay_gather_load_frames_shift, csrc/gather_common.cuh "the shifted pieces").

The yardstick is bit-equality and nothing else: `sample(indices=I, shifts=S)` of a buffer with random_shift equals
shift_cases.random_shift_reference — integer indexing in numpy — applied to `sample(indices=I)` of a twin buffer without it that was fed the same
stream, in both halves, the image and every sensor; every other field has the twin's bits.  The unaugmented batch is pinned by the tests of the
modes themselves.  S is shift_cases.injected_shifts: every shift of [-pad, pad]^2 in each half, and out-of-range entries up to the ends of
int32 (test_replay_shift_cpu.py checks the coverage condition).

Shapes (shift_cases.CONFIGS) are the smallest that reach every branch: a ring of T = 7 steps of 2 environments after 10 adds (pos = 3), frame
stacks 2 and 3; images 8 x 12 (the 16-byte form; H != W catches a dy / dx swap), 5 x 6 (the element form) and 4 x 4 with pad 4 (every lane an
edge lane, pad >= W); tactile 4 x 8 with 2 sensors and 3 x 5 with one (3 h w no multiple of 4); uint8 and float32 stores; pads 3 / 2 and 4 / 0."""
import numpy as np
import pytest
import torch

import memguard as MG
import shift_cases as SH

pytestmark = pytest.mark.gpu

import m3l_amd  # noqa: E402
from m3l_amd import _lib as L  # noqa: E402
from m3l_amd import replay as P  # noqa: E402

DEV = "cuda:0"
T, E, A = SH.T, SH.E, SH.A
RANGES = ((0.1, 0.9), (-2, 3))          # ranges floats cannot represent

# name -> the keywords of the buffer
MODES = {
    "two_stores": dict(),
    "single_store": dict(optimize_memory_usage=True, handle_timeout_termination=False),
    "dedup_two_stores": dict(frame_dedup=True),
    "dedup_single_store": dict(frame_dedup=True, optimize_memory_usage=True, handle_timeout_termination=False),
    "nstep3": dict(n_steps=3, gamma=0.97),
    "dedup_nstep3": dict(frame_dedup=True, n_steps=3, gamma=0.97),
    "prioritized": dict(prioritized=True),
}


def _buffer(cfg, **kw):
    fs, image_hw, tactile_hw, S, dtypes, _ = cfg
    shapes = {"image": (fs,) + image_hw + (3,), "tactile": (fs, 3 * S) + tactile_hw}
    return m3l_amd.DeviceReplayBuffer(T * E, E, shapes, {"image": dtypes[0], "tactile": dtypes[1]}, A, image_normalization=list(RANGES[0]),
                                      tactile_normalization=list(RANGES[1]), device=DEV, **kw)


def _fill(bufs, st, n_adds=SH.N_ADDS):
    for k in range(n_adds):
        for buf in bufs:
            buf.add({key: v[k] for key, v in st["obs"].items()}, {key: v[k] for key, v in st["next_obs"].items()}, st["actions"][k], st["rewards"][k],
                    st["dones"][k], st["infos"][k])
    for buf in bufs:
        assert buf.full and buf.pos == n_adds - T and 0 < buf.pos < T            # the ring has wrapped, pos mid-ring


def _indices(buf, B):
    """B valid (t, e) pairs, every valid pair of the buffer in turn."""
    first, count = buf._valid_steps()
    pairs = [((first + u) % T, e) for u in range(count) for e in range(E)]
    pairs = [pairs[i % len(pairs)] for i in range(B)]
    return np.array([p[0] for p in pairs]), np.array([p[1] for p in pairs])


def _check_half(got, plain, shifts, half, pads, what):
    want = SH.shifted_obs_reference({k: v.cpu().numpy() for k, v in plain.items()}, shifts, half, pads)
    assert isinstance(got, m3l_amd.LoadedObs) and sorted(got) == sorted(want), what
    for k, w in want.items():
        g = got[k].cpu().numpy()
        assert g.dtype == np.float32 and g.shape == w.shape, (what, k)
        bad = g.view(np.uint32) != np.ascontiguousarray(w).view(np.uint32)
        assert not bad.any(), f"{what}: {k} differs in {int(bad.sum())} of {bad.size} elements, first at {tuple(np.argwhere(bad)[0])}"


@pytest.mark.parametrize("name", sorted(SH.CONFIGS))
def test_augmented_batch_is_the_indexing_of_the_twins_batch(name):
    cfg = SH.CONFIGS[name]
    fs, image_hw, tactile_hw, S, dtypes, pads = cfg
    st = SH.make_stream(fs, image_hw, tactile_hw, S, dtypes[0], dtypes[1], seed=sorted(SH.CONFIGS).index(name))
    shifts = SH.injected_shifts(pads)
    d_shifts = torch.from_numpy(shifts).to(DEV)
    B = shifts.shape[0]
    for mode, kw in MODES.items():
        what = f"{name} {mode}"
        aug, twin = _buffer(cfg, random_shift=dict(image=pads[0], tactile=pads[1]), **kw), _buffer(cfg, **kw)
        _fill((aug, twin), st)
        idx = _indices(aug, B)
        got, plain = aug.sample(1, indices=idx, shifts=d_shifts), twin.sample(1, indices=idx)
        assert type(got) is type(plain) and got._fields == plain._fields, what
        assert aug.last_shifts is d_shifts
        assert not MG.nonfinite([dict(plain.observations), dict(plain.next_observations)]), what
        assert not torch.equal(got.observations["image"], plain.observations["image"]), what          # the shifts move something
        _check_half(got.observations, plain.observations, shifts, 0, pads, what + " observations")
        _check_half(got.next_observations, plain.next_observations, shifts, 1, pads, what + " next_observations")
        for fld in got._fields:
            if fld not in ("observations", "next_observations"):
                assert torch.equal(getattr(got, fld), getattr(plain, fld)), (what, fld)
        if "n_steps" in kw:
            assert (got.next_rows != got.rows).any(), what                  # some walk moved: the two halves come from different rows
        # the shifted form with zero shifts is the unaugmented batch, and two runs give the same bits
        zero = aug.sample(1, indices=idx, shifts=torch.zeros_like(d_shifts))
        assert not MG.differing(list(zero), list(plain)), what
        assert not MG.differing(list(got), list(aug.sample(1, indices=idx, shifts=d_shifts.clone()))), what


class _Recorder:
    """Stands where m3l_amd._lib keeps the loaded library and notes the entry points that are called."""

    def __init__(self, lib):
        self._lib, self.calls = lib, []

    def __getattr__(self, name):
        fn = getattr(self._lib, name)
        if not name.startswith("m3l_replay_"):
            return fn

        def call(*a):
            self.calls.append(name)
            return fn(*a)
        return call


@pytest.mark.parametrize("mode", ["two_stores", "dedup_two_stores", "nstep3", "dedup_nstep3"])
def test_off_is_off(mode, monkeypatch):
    """random_shift=None and all-zero pads: the twin's bits through the entry points of before, no shift tensor and no draw for one."""
    cfg = SH.CONFIGS["u8_8x12_f32_4x8_S2_fs2_pads32"]
    fs, image_hw, tactile_hw, S, dtypes, pads = cfg
    st = SH.make_stream(fs, image_hw, tactile_hw, S, dtypes[0], dtypes[1], seed=11)
    kw = MODES[mode]
    bufs = {"default": _buffer(cfg, **kw), "none": _buffer(cfg, random_shift=None, **kw), "zero": _buffer(cfg, random_shift=0, **kw),
            "zeros": _buffer(cfg, random_shift=dict(image=0, tactile=0), **kw), "on": _buffer(cfg, random_shift=dict(image=3, tactile=2), **kw)}
    _fill(list(bufs.values()), st)
    idx = _indices(bufs["default"], 9)
    rec = _Recorder(L.lib())
    monkeypatch.setattr(L, "_lib", rec)
    calls, out = {}, {}
    for key, buf in bufs.items():
        rec.calls = []
        out[key] = buf.sample(1, indices=idx)
        calls[key] = list(rec.calls)
    gather = "m3l_replay_gather_load" + ("_frames" if "dedup" in mode else "") + ("_rows2" if "nstep" in mode else "")
    scalars = "m3l_replay_nstep_rows" if "nstep" in mode else "m3l_replay_gather_rows"
    assert calls["default"] == [scalars, gather], calls["default"]
    for key in ("none", "zero", "zeros"):
        assert calls[key] == calls["default"], (key, calls[key])
        assert not MG.differing(list(out[key]), list(out["default"])), key
        assert bufs[key].last_shifts is None and bufs[key].random_shift is None
    assert calls["on"] == [scalars, "m3l_replay_gather_load" + ("_frames" if "dedup" in mode else "") + "_shift"], calls["on"]
    # the module functions: shifts without a pad, and pads without shifts, are the calls of before
    b = bufs["default"]
    rows = torch.from_numpy(idx[0] * E + idx[1]).to(DEV)
    some = torch.from_numpy(SH.injected_shifts((3, 2), 9)).to(DEV)
    if "dedup" in mode:
        call = lambda **k: P.gather_load_frames(b.frames["image"], b.frames["tactile"], b.ages, rows, b.next_frames["image"],       # noqa: E731
                                                b.next_frames["tactile"], *RANGES, frame_stack=fs, **k)
    else:
        call = lambda **k: P.gather_load(b.observations["image"], b.observations["tactile"], rows, b.next_observations["image"],    # noqa: E731
                                         b.next_observations["tactile"], *RANGES, **k)
    rec.calls = []
    base = call()
    for k in (dict(shifts=some), dict(shift_pad=(3, 2)), dict(shifts=some, shift_pad=(0, 0))):
        assert not MG.differing([dict(x) for x in call(**k)], [dict(x) for x in base]), k
    assert set(rec.calls) == {gather.replace("_rows2", "")}, rec.calls


@pytest.mark.parametrize("name", ["u8_8x12_f32_4x8_S2_fs2_pads32", "f32_5x6_u8_3x5_S1_fs3_pads32"])
def test_a_wrong_row_gives_nan_and_changes_nothing_else(name):
    cfg = SH.CONFIGS[name]
    fs, image_hw, tactile_hw, S, dtypes, pads = cfg
    st = SH.make_stream(fs, image_hw, tactile_hw, S, dtypes[0], dtypes[1], seed=21)
    sbuf, dbuf = _buffer(cfg), _buffer(cfg, frame_dedup=True)
    _fill((sbuf, dbuf), st)
    t, e = _indices(dbuf, 9)
    rows = torch.from_numpy(t * E + e).to(DEV)
    shifts = torch.from_numpy(SH.injected_shifts(pads, 9)).to(DEV)
    bad_rows = rows.clone()
    bad_rows[1], bad_rows[4], bad_rows[7] = -1, T * E, -2 ** 40
    wrong = torch.tensor([i in (1, 4, 7) for i in range(9)], device=DEV)

    def gathers(r, **k):
        so, sn, do, dn = sbuf.observations, sbuf.next_observations, dbuf.frames, dbuf.next_frames
        return (P.gather_load(so["image"], so["tactile"], r, sn["image"], sn["tactile"], *RANGES, shifts=shifts, shift_pad=pads, **k),
                P.gather_load_frames(do["image"], do["tactile"], dbuf.ages, r, dn["image"], dn["tactile"], *RANGES, shifts=shifts, shift_pad=pads,
                                     frame_stack=fs, **k))
    want = gathers(rows)
    assert not MG.differing([dict(x) for x in want[0]], [dict(x) for x in want[1]]) and not MG.nonfinite([dict(x) for x in want[0]])
    for halves, whalves, form in zip(gathers(bad_rows), want, ("stacked", "frames")):
        for half, whalf in zip(halves, whalves):
            for key in whalf:
                assert torch.isnan(half[key][wrong]).all() and torch.equal(half[key][~wrong], whalf[key][~wrong]), (form, key)
    # a second row list: a wrong entry blanks its own half alone
    for (obs, nob), (wobs, wnob), form in zip(gathers(rows, next_rows=bad_rows), gathers(rows, next_rows=rows), ("stacked", "frames")):
        for key in wobs:
            assert torch.equal(obs[key], wobs[key]), (form, key)
            assert torch.isnan(nob[key][wrong]).all() and torch.equal(nob[key][~wrong], wnob[key][~wrong]), (form, key)
    # next_rows = rows is the one-list form, and a row shift on the rows side is the shift applied on the host
    assert not MG.differing([dict(x) for g in gathers(rows, next_rows=rows) for x in g], [dict(x) for g in want for x in g])
    every = torch.arange(9, dtype=torch.int64, device=DEV)
    assert not MG.differing([dict(x) for g in gathers(every, row_shift=5) for x in g], [dict(x) for g in gathers((every + 5) % (T * E)) for x in g])


def test_drawn_shifts():
    """B = 4096 with pads 2 and 1: what `sample()` draws on the device.  A value missing from one of the 8 components has a chance below
    8 * 5 * (4/5)^8192 < 1e-300."""
    cfg = SH.CONFIGS["u8_8x12_f32_4x8_S2_fs2_pads32"]
    fs, image_hw, tactile_hw, S, dtypes, _ = cfg
    st = SH.make_stream(fs, image_hw, tactile_hw, S, dtypes[0], dtypes[1], seed=31)
    pads = (2, 1)
    buf, same = _buffer(cfg, random_shift=dict(image=2, tactile=1)), _buffer(cfg, random_shift=2)
    _fill((buf, same), st)
    B = 4096
    torch.manual_seed(5)
    batch = buf.sample(B)
    s = buf.last_shifts
    assert s.shape == (B, 2, 2, 2) and s.dtype == torch.int32 and s.is_cuda and s.is_contiguous()
    host = s.cpu().numpy()
    for m, p in enumerate(pads):
        for half in (0, 1):
            for c in (0, 1):
                assert sorted(set(host[:, half, m, c].tolist())) == list(range(-p, p + 1)), (m, half, c)
    assert (host[:, 0] != host[:, 1]).any()
    rows = batch.rows.cpu()
    again = buf.sample(1, indices=(rows // E, rows % E), shifts=s)
    assert not MG.differing(list(batch), list(again)) and not MG.nonfinite(list(batch))
    plain = buf.sample(1, indices=(rows // E, rows % E), shifts=torch.zeros_like(s))
    _check_half(batch.observations, plain.observations, host, 0, pads, "drawn observations")
    _check_half(batch.next_observations, plain.next_observations, host, 1, pads, "drawn next_observations")
    torch.manual_seed(5)
    buf.sample(B)
    assert buf.last_shifts is not s and torch.equal(buf.last_shifts, s)
    # equal pads: one draw over the whole tensor, every entry in range
    same.sample(B)
    eq = same.last_shifts.cpu().numpy()
    assert eq.shape == (B, 2, 2, 2) and eq.min() == -2 and eq.max() == 2
    with pytest.raises(ValueError, match=r"shifts must be a contiguous int32 tensor of shape \(B, 2, 2, 2\) = \(8, 2, 2, 2\)"):
        buf.sample(8, shifts=s)
