"""DeviceRolloutBuffer's random shift and frame store on a real MI355X (m3l_amd/rollout.py `random_shift=`, `frame_dedup=`; csrc/rollout.hip
m3l_rollout_gather_load_shift / _frames / _frames_shift; csrc/gather_common.cuh "the shifted pieces", rollout_frame_slot).

The yardstick is bit-equality and nothing else.  Shift: `get(indices=I, shifts=S)` of a buffer with random_shift equals
shift_cases.random_shift_reference — integer indexing in numpy — applied to `get(indices=I)` of a twin without it that was fed the same stream.
Frame store: the batches of a frame_dedup buffer equal those of a stacked buffer fed the same stream, and rollout_cases.feed_reference on the host
stores.  S is rollout_aug_cases.injected_shifts: every shift of [-pad, pad]^2 and out-of-range entries up to the ends of int32.

Shapes (shift_cases.CONFIGS) are the smallest that reach every branch: rollouts of T = 5 and 7 steps of 2 environments, two consecutive ones with
a reset() between (the second begins at an episode start, inside a young episode and inside an old one: test_rollout_aug_cpu.py), frame stacks 2
and 3; images 8 x 12 (the 16-byte form; H != W), 5 x 6 (the element form) and 4 x 4 with pad 4 (pad >= W); tactile 4 x 8 with 2 sensors and 3 x 5
with one (3 h w no multiple of 4); uint8 and float32 stores; pads 3 / 2 and 4 / 0."""
import numpy as np
import pytest
import torch

import memguard as MG
import rollout_aug_cases as RA
import rollout_cases as RC
import shift_cases as SH

pytestmark = pytest.mark.gpu

import m3l_amd  # noqa: E402
from m3l_amd import _lib as L  # noqa: E402
from m3l_amd import rollout as R  # noqa: E402

DEV = "cuda:0"
E, A = RA.E, RA.A
RANGES = ((0.1, 0.9), (-2, 3))          # ranges floats cannot represent
SCALARS = ("actions", "old_values", "old_log_prob", "advantages", "returns")


def _buffer(name, T, **kw):
    fs, image_hw, tactile_hw, S, dtypes, _ = RA.CONFIGS[name]
    shapes = {"image": (fs,) + image_hw + (3,), "tactile": (fs, 3 * S) + tactile_hw}
    return m3l_amd.DeviceRolloutBuffer(T, E, shapes, {"image": dtypes[0], "tactile": dtypes[1]}, A, image_normalization=list(RANGES[0]),
                                       tactile_normalization=list(RANGES[1]), device=DEV, **kw)


def _feed(bufs, ro, r, obs=None):
    """Rollout r of the stream into every buffer: reset(), T add() calls, the returns."""
    obs = ro["obs"] if obs is None else obs
    sl = RA.rollout_slice(ro, r)
    for buf in bufs:
        buf.reset()
        for k in range(sl.start, sl.stop):
            buf.add({key: v[k] for key, v in obs.items()}, ro["actions"][k], ro["rewards"][k], ro["episode_start"][k], ro["values"][k], ro["log_probs"][k])
        assert buf.full
        buf.compute_returns_and_advantage(ro["last_values"][r], ro["dones"][r])


def _one(gen):
    batches = list(gen)
    assert len(batches) == 1
    return batches[0]


def _bits_equal(got, want, what):
    assert sorted(got) == sorted(want), what
    for k, w in want.items():
        g = got[k].cpu().numpy() if isinstance(got[k], torch.Tensor) else got[k]
        w = w.cpu().numpy() if isinstance(w, torch.Tensor) else np.ascontiguousarray(w)
        assert g.dtype == np.float32 and w.dtype == np.float32 and g.shape == w.shape, (what, k)
        bad = g.view(np.int32) != w.view(np.int32)
        assert not bad.any(), f"{what}: {k} differs in {int(bad.sum())} of {bad.size} elements, first at {tuple(np.argwhere(bad)[0])}"


# ---- 1. shift parity
@pytest.mark.parametrize("name", sorted(RA.CONFIGS))
def test_augmented_batch_is_the_indexing_of_the_twins_batch(name):
    pads = RA.CONFIGS[name][5]
    shifts = RA.injected_shifts(pads)
    d_shifts = torch.from_numpy(shifts).to(DEV)
    N = shifts.shape[0]
    for T in RA.ROLLOUT_T:
        ro = RA.make_rollouts(name, T, seed=sorted(RA.CONFIGS).index(name))
        idx = np.arange(N) % (T * E)          # every flat index, repeated to the length of the shift list
        for dedup in (False, True):
            what = f"{name} T={T} {'frame_dedup' if dedup else 'stacked'}"
            aug, twin = _buffer(name, T, frame_dedup=dedup, random_shift=dict(image=pads[0], tactile=pads[1])), _buffer(name, T, frame_dedup=dedup)
            for r in (0, 1):
                _feed((aug, twin), ro, r)
                got, plain = _one(aug.get(indices=idx, shifts=d_shifts)), _one(twin.get(indices=idx))
                assert type(got) is m3l_amd.RolloutBatch and isinstance(got.x, m3l_amd.LoadedObs) and got.observations is got.x, what
                assert aug.last_shifts is d_shifts and twin.last_shifts is None
                assert not MG.nonfinite(dict(plain.x)), what
                assert not torch.equal(got.x["image"], plain.x["image"]), what          # the shifts move something
                _bits_equal(dict(got.x), RA.shifted_reference({k: v.cpu().numpy() for k, v in plain.x.items()}, shifts, pads), f"{what} rollout {r}")
                for fld in SCALARS:
                    assert torch.equal(getattr(got, fld), getattr(plain, fld)), (what, fld)
            # minibatches take their slices of the injected list; zero shifts are the unaugmented batch; two runs give the same bits
            parts = list(aug.get(batch_size=N // 3 + 1, indices=idx, shifts=d_shifts))
            assert len(parts) == 3 and aug.last_shifts.shape[0] == N - 2 * (N // 3 + 1)
            assert not MG.differing({k: torch.cat([p.x[k] for p in parts]) for k in got.x}, dict(got.x)), what
            zero = _one(aug.get(indices=idx, shifts=torch.zeros_like(d_shifts)))
            assert not MG.differing(list(zero), list(plain)), what
            assert not MG.differing(list(got), list(_one(aug.get(indices=idx, shifts=d_shifts.clone())))), what


# ---- 2. frame-store parity
@pytest.mark.parametrize("name", sorted(RA.CONFIGS))
def test_frame_store_gives_the_stacked_buffers_batches(name):
    fs = RA.CONFIGS[name][0]
    for T in RA.ROLLOUT_T:
        ro = RA.make_rollouts(name, T, seed=40 + sorted(RA.CONFIGS).index(name))
        stacked, dedup = _buffer(name, T), _buffer(name, T, frame_dedup=True, check_stacking=True)
        idx = np.concatenate([np.arange(T * E), np.arange(T * E)[::-1]])          # every flat index, both ways
        for r in (0, 1):
            what = f"{name} T={T} rollout {r}"
            _feed((stacked, dedup), ro, r)
            assert dedup.observations is None and stacked.frames is None and stacked.ages is None
            assert {k: tuple(v.shape) for k, v in dedup.frames.items()} == {k: (T + fs - 1, E) + s[1:] for k, s in dedup.obs_shapes.items()}
            sl = RA.rollout_slice(ro, r)
            # the stores are what the restatement says add() stores
            for key in ("image", "tactile"):
                frames, ages = RA.frame_store_reference(ro["obs"][key][sl], ro["episode_start"][sl], fs)
                assert np.array_equal(dedup.frames[key].cpu().numpy(), frames) and np.array_equal(dedup.ages.cpu().numpy(), ages), (what, key)
            a, b = _one(stacked.get(indices=idx)), _one(dedup.get(indices=idx))
            assert not MG.differing(list(b), list(a)) and not MG.nonfinite(list(a)), what
            want = RC.feed_reference({k: v[sl] for k, v in ro["obs"].items()}, idx, *RANGES)
            _bits_equal(dict(b.x), want, what)
            # minibatches of a drawn permutation: the same rows through both stores
            torch.manual_seed(7)
            pa = list(stacked.get(batch_size=T))
            torch.manual_seed(7)
            pb = list(dedup.get(batch_size=T))
            assert len(pa) == E and not MG.differing([list(x) for x in pb], [list(x) for x in pa]), what
        assert dedup.store_bytes()["observations"] == sum(v.numel() * v.element_size() for v in dedup.frames.values())
        assert stacked.store_bytes()["observations"] == sum(v.numel() * v.element_size() for v in stacked.observations.values())


# ---- 3. off is off
class _Recorder:
    """Stands where m3l_amd._lib keeps the loaded library and notes the entry points that are called."""

    def __init__(self, lib):
        self._lib, self.calls = lib, []

    def __getattr__(self, name):
        fn = getattr(self._lib, name)
        if not name.startswith("m3l_rollout_"):
            return fn

        def call(*a):
            self.calls.append(name)
            return fn(*a)
        return call


def test_off_is_off(monkeypatch):
    """random_shift=None, all-zero pads and frame_dedup=False: m3l_rollout_gather_load alone, no shift tensor and no draw for one."""
    name, T = "u8_8x12_f32_4x8_S2_fs2_pads32", 5
    ro = RA.make_rollouts(name, T, seed=11)
    off = {"default": _buffer(name, T), "none": _buffer(name, T, random_shift=None, frame_dedup=False), "zero": _buffer(name, T, random_shift=0),
           "zeros": _buffer(name, T, random_shift=dict(image=0, tactile=0))}
    on = {"_shift": _buffer(name, T, random_shift=dict(image=3, tactile=2)), "_frames": _buffer(name, T, frame_dedup=True),
          "_frames_shift": _buffer(name, T, frame_dedup=True, random_shift=2), "_frames_zero": _buffer(name, T, frame_dedup=True, random_shift=0)}
    _feed(list(off.values()) + list(on.values()), ro, 0)
    idx = np.arange(T * E)
    rec = _Recorder(L.lib())
    monkeypatch.setattr(L, "_lib", rec)
    out = {}
    for key, buf in {**off, **on}.items():
        rec.calls = []
        out[key] = _one(buf.get(indices=idx))
        suffix = "" if key in off else key.replace("_zero", "")
        assert rec.calls == ["m3l_rollout_gather_load" + suffix, "m3l_rollout_gather_rows"], (key, rec.calls)
    for key, buf in off.items():
        assert not MG.differing(list(out[key]), list(out["default"])), key
        assert buf.last_shifts is None and buf.random_shift is None
    assert not MG.differing(list(out["_frames"]), list(out["default"])) and not MG.differing(list(out["_frames_zero"]), list(out["default"]))
    assert on["_frames_zero"].last_shifts is None and on["_shift"].last_shifts is not None
    # zero shifts through the shifted entry points give the unaugmented bits
    zeros = torch.zeros(T * E, 2, 2, dtype=torch.int32, device=DEV)
    for key in ("_shift", "_frames_shift"):
        rec.calls = []
        assert not MG.differing(list(_one(on[key].get(indices=idx, shifts=zeros))), list(out["default"])), key
        assert rec.calls[0] == "m3l_rollout_gather_load" + key
    # the module functions: shifts without a pad, and pads without shifts, are the calls of before
    b, d = off["default"], on["_frames"]
    d_idx = torch.from_numpy(idx).to(DEV)
    some = torch.from_numpy(RA.injected_shifts((3, 2))[:T * E]).to(DEV)
    for call, entry in ((lambda **k: R.gather_load(b.observations["image"], b.observations["tactile"], d_idx, *RANGES, **k), "m3l_rollout_gather_load"),
                        (lambda **k: R.gather_load_frames(d.frames["image"], d.frames["tactile"], d.ages, d_idx, 2, *RANGES, **k),
                         "m3l_rollout_gather_load_frames")):
        rec.calls = []
        for k in (dict(), dict(shifts=some), dict(shift_pad=(3, 2)), dict(shifts=some, shift_pad=(0, 0))):
            assert not MG.differing(dict(call(**k)), dict(out["default"].x)), (entry, k)
        assert set(rec.calls) == {entry}, rec.calls
        rec.calls = []
        assert MG.differing(dict(call(shifts=some, shift_pad=(3, 2))), dict(out["default"].x)) and rec.calls == [entry + "_shift"]
    # an image-only store: the tactile pad shifts nothing
    rec.calls = []
    R.gather_load(b.observations["image"], None, d_idx, *RANGES, shifts=some, shift_pad=(0, 2))
    assert rec.calls == ["m3l_rollout_gather_load"]


# ---- 4. wrong indices and ages
@pytest.mark.parametrize("name", ["u8_8x12_f32_4x8_S2_fs2_pads32", "f32_5x6_u8_3x5_S1_fs3_pads32"])
def test_wrong_indices_give_nan_rows_and_any_age_is_clamped(name):
    fs, pads, T = RA.CONFIGS[name][0], RA.CONFIGS[name][5], 7
    ro = RA.make_rollouts(name, T, seed=21)
    sbuf, dbuf = _buffer(name, T), _buffer(name, T, frame_dedup=True)
    _feed((sbuf, dbuf), ro, 0)
    _feed((sbuf, dbuf), ro, 1)
    idx = torch.arange(T * E, dtype=torch.int64, device=DEV)
    shifts = torch.from_numpy(RA.injected_shifts(pads)[:T * E]).to(DEV)
    bad_idx = idx.clone()
    bad_idx[1], bad_idx[4], bad_idx[7], bad_idx[9] = -1, T * E, -2 ** 40, 2 ** 31
    wrong = torch.tensor([i in (1, 4, 7, 9) for i in range(T * E)], device=DEV)
    so, fr = sbuf.observations, dbuf.frames

    def gathers(i, ages=dbuf.ages, **k):
        return (R.gather_load(so["image"], so["tactile"], i, *RANGES, **k), R.gather_load_frames(fr["image"], fr["tactile"], ages, i, fs, *RANGES, **k))
    for kw in (dict(), dict(shifts=shifts, shift_pad=pads)):
        want = gathers(idx, **kw)
        assert not MG.differing(dict(want[0]), dict(want[1])) and not MG.nonfinite(dict(want[0]))
        for got, w, form in zip(gathers(bad_idx, **kw), want, ("stacked", "frames")):
            for key in w:
                assert torch.isnan(got[key][wrong]).all() and torch.equal(got[key][~wrong], w[key][~wrong]), (form, key, sorted(kw))
    # ages: negative, huge and the ends of int32 give the batch of the clamped ages
    host = dbuf.ages.cpu().numpy().copy()
    wild = np.array([SH.INT32_MIN, -1, -1000, 0, 1, fs - 1, fs, 1000, SH.INT32_MAX, SH.INT32_MIN + 1, SH.INT32_MAX - 1, 2, fs - 2, -fs], dtype=np.int64)
    wild = np.resize(wild, T * E).reshape(T, E).astype(np.int32)
    clamped = np.clip(wild, 0, fs - 1).astype(np.int32)
    assert (wild != clamped).any() and (clamped != host).any()
    for kw in (dict(), dict(shifts=shifts, shift_pad=pads)):
        a = R.gather_load_frames(fr["image"], fr["tactile"], torch.from_numpy(wild).to(DEV), idx, fs, *RANGES, **kw)
        b = R.gather_load_frames(fr["image"], fr["tactile"], torch.from_numpy(clamped).to(DEV), idx, fs, *RANGES, **kw)
        assert not MG.differing(dict(a), dict(b)) and not MG.nonfinite(dict(a))
        if not kw:          # and that batch is the slot rule's, read out of the host copy of the frames
            stores = {k: RA.stacked_from_frames(v.cpu().numpy(), clamped, fs) for k, v in fr.items()}
            _bits_equal(dict(a), RC.feed_reference(stores, idx.cpu().numpy(), *RANGES), name)


# ---- 5. drawn shifts
def test_drawn_shifts():
    """B = 4096 with pads 2 and 1: what `get()` draws on the device.  A value missing from one of the 4 components has a chance below
    4 * 5 * (4/5)^4096 < 1e-390."""
    name, T, B, pads = "u8_8x12_f32_4x8_S2_fs2_pads32", 5, 4096, (2, 1)
    ro = RA.make_rollouts(name, T, seed=31)
    buf, same, img_only = _buffer(name, T, random_shift=dict(image=2, tactile=1)), _buffer(name, T, frame_dedup=True, random_shift=2), \
        _buffer(name, T, random_shift=dict(image=2))
    _feed((buf, same, img_only), ro, 0)
    idx = np.arange(B) % (T * E)
    torch.manual_seed(5)
    batch = _one(buf.get(indices=idx))
    s = buf.last_shifts
    assert s.shape == (B, 2, 2) and s.dtype == torch.int32 and s.device == buf.observations["image"].device and s.is_contiguous()
    host = s.cpu().numpy()
    for m, p in enumerate(pads):
        for c in (0, 1):
            assert sorted(set(host[:, m, c].tolist())) == list(range(-p, p + 1)), (m, c)
    again = _one(buf.get(indices=idx, shifts=s))
    assert buf.last_shifts is s and not MG.differing(list(batch), list(again)) and not MG.nonfinite(list(batch))
    plain = _one(buf.get(indices=idx, shifts=torch.zeros_like(s)))
    _bits_equal(dict(batch.x), RA.shifted_reference({k: v.cpu().numpy() for k, v in plain.x.items()}, host, pads), "drawn")
    torch.manual_seed(5)
    _one(buf.get(indices=idx))
    assert buf.last_shifts is not s and torch.equal(buf.last_shifts, s)
    # every minibatch draws its own; the last batch's tensor is kept
    sizes = [b.actions.shape[0] for b in buf.get(batch_size=1500, indices=idx)]
    assert sizes == [1500, 1500, 1096] and buf.last_shifts.shape == (1096, 2, 2)
    # equal pads: one draw over the whole tensor; a zero-pad modality keeps zeros
    _one(same.get(indices=idx))
    eq = same.last_shifts.cpu().numpy()
    assert eq.shape == (B, 2, 2) and eq.min() == -2 and eq.max() == 2
    _one(img_only.get(indices=idx))
    z = img_only.last_shifts.cpu().numpy()
    assert (z[:, 1] == 0).all() and sorted(set(z[:, 0].ravel().tolist())) == [-2, -1, 0, 1, 2]
    with pytest.raises(ValueError, match=r"shifts must be a contiguous int32 tensor of shape \(B, 2, 2\) = \(8, 2, 2\)"):
        buf.get(indices=idx[:8], shifts=s)
    with pytest.raises(ValueError, match="indices outside"):
        buf.get(indices=[0, T * E], shifts=s[:2].contiguous())


# ---- 6. check_stacking
def test_check_stacking():
    name, T = "f32_5x6_u8_3x5_S1_fs3_pads32", 7
    ro = RA.make_rollouts(name, T, seed=51)
    buf = _buffer(name, T, frame_dedup=True, check_stacking=True)
    _feed((buf,), ro, 0)
    _feed((buf,), ro, 1)          # the contract holds across the reset()
    # one frame altered: an older frame of a mid-episode stack, and a frame of an episode's first stack
    start = ro["episode_start"]
    k_mid, e_mid = next((k, e) for k in range(1, T) for e in range(E) if not start[k, e])
    k_first, e_first = next((k, e) for k in range(1, T) for e in range(E) if start[k, e])
    for key, k, e, j, rule in (("image", k_mid, e_mid, 0, r"obs\[:, :-1\] equals the previous add\(\)'s obs\[:, 1:\]"),
                               ("tactile", k_first, e_first, 1, "all frames of obs are equal at an episode's first step")):
        obs = {kk: v.copy() for kk, v in ro["obs"].items()}
        obs[key][k, e, j].flat[3] += 1
        fresh = _buffer(name, T, frame_dedup=True, check_stacking=True)
        with pytest.raises(ValueError, match=rf"check_stacking: observation '{key}' of environment {e} breaks the contract of frame_dedup=True: {rule}"):
            _feed((fresh,), ro, 0, obs)
        assert fresh.pos == k          # the steps before it were taken
        # without the check the altered stream is stored as it comes
        _feed((_buffer(name, T, frame_dedup=True),), ro, 0, obs)
    # episode_start lives on the host
    fresh = _buffer(name, T, frame_dedup=True)
    with pytest.raises(ValueError, match="frame_dedup=True follows the episodes on the host and needs `episode_start` there"):
        fresh.add({key: v[0] for key, v in ro["obs"].items()}, ro["actions"][0], ro["rewards"][0], torch.ones(E, device=DEV), ro["values"][0], ro["log_probs"][0])
    assert fresh.frames is None and fresh.pos == 0
