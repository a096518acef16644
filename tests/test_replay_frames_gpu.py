"""The frame-deduplicated replay store on a real MI355X (m3l_amd/replay.py `frame_dedup=True`, csrc/replay.hip m3l_replay_gather_load_frames).

The yardstick is the stacked DeviceReplayBuffer, which test_replay_gpu.py holds to the reference's recorded minibatches: one stream of add()
calls — the rolling stacks of FrameStack-wrapped environments with auto-reset, restated in tests/replay_frame_cases.py — goes into a stacked
buffer and into a deduplicated one, and `sample(indices=...)` over every valid (t, e) of the deduplicated buffer must give equal bits.  Both
are also held to replay_cases.sample_reference on the numpy stacks and to the restated frame rule.  In the single-store mode a step that ended
its episode has no agreed next observation (the stacked store returns the new episode's reset stack, the deduplicated one the old episode's
frames and the reset frame; SB3 multiplies either by 1 - done), so there next_observations is compared to the stacked buffer where done = 0 and
to the restated rule everywhere.  Everything is a copy or (x - lo) / span of one element: equal bits, no tolerance.

Shapes are the smallest that reach every path: T = 7 steps of 2 environments, frame stacks 1..4 (episodes of 1, 2, fs - 1 and fs + 2 steps),
pixel counts that are and are not a multiple of the 4-element vector, one to four sensors."""
import re

import numpy as np
import pytest
import torch

import memguard as MG
import replay_cases as PC
import replay_frame_cases as FC
import rollout_cases as RC

pytestmark = pytest.mark.gpu

import m3l_amd  # noqa: E402
from m3l_amd import replay as P  # noqa: E402

DEV = "cuda:0"
T, E, A = 7, 2, 3
U8, F32 = np.uint8, np.float32
CHECKPOINTS = (5, 7, 17)          # not full; just full (pos = 0); wrapped more than twice (pos = 3)


def _dev(stores):
    return None if stores is None else {k: torch.from_numpy(np.ascontiguousarray(v)).to(DEV) for k, v in stores.items()}


def _assert_same(got, want, what, keep=None):
    assert sorted(got) == sorted(want), what
    for k in want:
        w = want[k] if isinstance(want[k], torch.Tensor) else torch.from_numpy(np.ascontiguousarray(want[k])).to(DEV)
        g = got[k]
        assert g.dtype == torch.float32 and g.is_cuda and g.shape == w.shape, (what, k)
        if keep is not None:
            g, w = g[keep], w[keep]
        assert torch.equal(g, w), f"{what}: {k} differs in {(g != w).sum().item()} of {w.numel()} elements"


def _buffers(fs, single, image_hw, tactile_hw, S, dtypes, img_range=(0, 1), tac_range=(-1, 1), stacked=True, **kw):
    shapes, dts = {}, {}
    if image_hw is not None:
        shapes["image"], dts["image"] = (fs,) + tuple(image_hw) + (3,), dtypes[0]
    if tactile_hw is not None:
        shapes["tactile"], dts["tactile"] = (fs, 3 * S) + tuple(tactile_hw), dtypes[1]
    args = dict(optimize_memory_usage=single, handle_timeout_termination=not single, image_normalization=list(img_range),
                tactile_normalization=list(tac_range), device=DEV)
    sbuf = m3l_amd.DeviceReplayBuffer(T * E, E, shapes, dts, A, **args) if stacked else None
    return sbuf, m3l_amd.DeviceReplayBuffer(T * E, E, shapes, dts, A, frame_dedup=True, **args, **kw)


def _add(buf, st, k):
    buf.add({key: v[k] for key, v in st["obs"].items()}, {key: v[k] for key, v in st["next_obs"].items()}, st["actions"][k], st["rewards"][k],
            st["dones"][k], st["infos"][k])


def _check_batch(batch, ref, t, e, n, st, fs, single, ranges, what):
    """`batch` of the deduplicated buffer for steps (t, e) after n adds against: `ref`, the stacked buffer's batch for the same indices;
    sample_reference on the numpy stacks; the restated frame rule."""
    stacked_m, model = FC.fill_models(n, T, fs, single, st)
    assert isinstance(batch, m3l_amd.ReplayBatch) and isinstance(batch.observations, m3l_amd.LoadedObs)
    k = np.array([model.step[x] for x in t])
    keep = None if not single else torch.from_numpy(~st["dones"][k, e]).to(DEV)      # single store: next observations agree where done = 0
    for name in ("actions", "rewards", "dones", "rows"):
        assert torch.equal(getattr(batch, name), getattr(ref, name)), (what, name)
    _assert_same(batch.observations, dict(ref.observations), what + " observations vs the stacked buffer")
    _assert_same(batch.next_observations, dict(ref.next_observations), what + " next_observations vs the stacked buffer", keep)
    stores, nstores, scalars = FC.stacked_stores(stacked_m, st)
    want = PC.sample_reference(stores, nstores, scalars, t, e, T, None, *ranges)
    _assert_same(batch.observations, want["observations"], what + " observations vs the numpy restatement")
    _assert_same(batch.next_observations, want["next_observations"], what + " next_observations vs the numpy restatement", keep)
    for name in ("actions", "dones", "rewards", "rows"):
        assert torch.equal(getattr(batch, name).cpu(), torch.from_numpy(np.ascontiguousarray(want[name]))), (what, name)
    exp_obs, exp_next = FC.expected_from_model(model, st, t, e, *ranges)
    _assert_same(batch.observations, exp_obs, what + " observations vs the restated frame rule")
    _assert_same(batch.next_observations, exp_next, what + " next_observations vs the restated frame rule")
    return 0 if keep is None else int((~keep).sum())


def _check_equivalence(n, sbuf, dbuf, st, fs, single, ranges=((0, 1), (-1, 1))):
    """Every valid (t, e) after n adds; the valid set against the pure-Python model; the steps just outside raise."""
    _, model = FC.fill_models(n, T, fs, single, st)
    assert (dbuf.pos, dbuf.full, dbuf.size()) == (model.pos, model.full, model.size()) == (sbuf.pos, sbuf.full, sbuf.size())
    valid = model.valid_steps()
    first, count = dbuf._valid_steps()
    assert [(first + u) % T for u in range(count)] == valid and count >= 1
    ages = dbuf.ages.cpu()
    assert ages.dtype == torch.int32 and all(ages[s].tolist() == model.ages[s] for s in range(T) if model.ages[s] is not None)
    t, e = np.repeat(valid, E), np.tile(np.arange(E), len(valid))
    n_caveat = _check_batch(dbuf.sample(1, indices=(t, e)), sbuf.sample(1, indices=(t, e)), t, e, n, st, fs, single, ranges, f"after {n} adds")
    outside = [s for s in range(T) if s not in valid]
    assert len(outside) == (T - n if n < T else fs - 1 + int(single))
    for s in outside:
        with pytest.raises(ValueError, match="indices name steps outside"):
            dbuf.sample(1, indices=([valid[0], s], [0, E - 1]))
    return n_caveat


def _run(fs, single, image_hw, tactile_hw, S, dtypes, seed, ranges=((0, 1), (-1, 1)), checkpoints=CHECKPOINTS):
    st = FC.make_stream(max(checkpoints), E, fs, image_hw, tactile_hw, S, dtypes[0], dtypes[1], A, seed)
    sbuf, dbuf = _buffers(fs, single, image_hw, tactile_hw, S, dtypes, *ranges)
    n_caveat = 0
    for k in range(max(checkpoints)):
        _add(sbuf, st, k)
        _add(dbuf, st, k)
        if k + 1 in checkpoints:
            n_caveat += _check_equivalence(k + 1, sbuf, dbuf, st, fs, single, ranges)
    assert dbuf.observations is None and dbuf.next_observations is None and (dbuf.next_frames is None) == single
    return n_caveat


@pytest.mark.parametrize("dtypes", [(U8, F32), (F32, F32), (F32, U8)], ids=["u8_f32", "f32_f32", "f32_u8"])
@pytest.mark.parametrize("single", [False, True], ids=["two_stores", "single_store"])
@pytest.mark.parametrize("fs", [1, 2, 3, 4])
def test_dedup_buffer_equals_the_stacked_buffer(fs, single, dtypes):
    """Case 1: image 8 x 8, tactile 4 x 4, S = 2 (the 16-byte paths), after 5, 7 and 17 adds."""
    n_caveat = _run(fs, single, (8, 8), (4, 4), 2, dtypes, seed=100 * fs + 10 * single)
    # the streams end episodes often enough that the single-store caveat is met, not only allowed for
    assert not single or n_caveat > 0


@pytest.mark.parametrize("single", [False, True], ids=["two_stores", "single_store"])
@pytest.mark.parametrize("image_hw,tactile_hw,S,dtypes,ranges", [
    ((6, 10), (5, 3), 1, (U8, F32), ((0, 1), (-1, 1))),              # 60 pixels: vectors; 45 tactile elements: element-wise
    ((5, 5), (5, 3), 4, (F32, U8), ((0.1, 0.3), (-2, 3))),           # 25 pixels: element-wise; four sensors; ranges floats cannot represent
    ((5, 5), (4, 4), 4, (U8, F32), ((0, 255), (-0.7, 0.9))),
    ((5, 5), None, 0, (U8, None), ((0, 255), (-1, 1))),              # image only
    ((8, 8), None, 0, (F32, None), ((0, 1), (-1, 1))),
    (None, (5, 3), 4, (None, F32), ((0, 1), (-0.7, 0.9))),           # tactile only
    (None, (4, 4), 1, (None, U8), ((0, 1), (-2, 3))),
], ids=["6x10_5x3_S1", "5x5_5x3_S4", "5x5_4x4_S4", "image_5x5", "image_8x8", "tactile_5x3_S4", "tactile_4x4_S1"])
def test_element_wise_paths_single_modalities_and_ranges(image_hw, tactile_hw, S, dtypes, ranges, single):
    """Case 2, with fs = 3 after 7 and 17 adds."""
    _run(3, single, image_hw, tactile_hw, S, dtypes, seed=200 + S + single, ranges=ranges, checkpoints=(7, 17))


# ---- the entry point called directly
def _direct(fs, image_hw, tactile_hw, S, dtypes, seed):
    frames = FC.make_frame_stores(T, E, image_hw, tactile_hw, S, dtypes[0], dtypes[1], seed)
    nxt = FC.make_frame_stores(T, E, image_hw, tactile_hw, S, dtypes[0], dtypes[1], seed + 1)
    ages = np.random.default_rng(seed).integers(0, fs, (T, E)).astype(np.int32)
    return frames, nxt, ages


def _call(dframes, dnext, dages, rows, fs, **kw):
    dn = dnext or {}
    return P.gather_load_frames(dframes.get("image"), dframes.get("tactile"), dages, rows, dn.get("image"), dn.get("tactile"), frame_stack=fs, **kw)


@pytest.mark.parametrize("image_hw,tactile_hw,S,dtypes", [((8, 8), (4, 4), 2, (U8, F32)), ((5, 5), (5, 3), 3, (F32, U8))], ids=["vector", "element_wise"])
def test_gather_load_frames_ages_rows_and_row_shift(image_hw, tactile_hw, S, dtypes):
    """Case 3.  Ages outside [0, fs - 1] give the bits of the clamped ages; rows outside [0, T n_envs) give NaN samples and leave the others
    intact; every row_shift agrees with rows shifted on the host.  All against the numpy restatement, in both store modes."""
    fs, n = 4, T * E
    frames, nxt, ages = _direct(fs, image_hw, tactile_hw, S, dtypes, seed=31)
    wild = ages.copy()
    wild[ages == 0] = -3
    wild[ages == fs - 1] = 100
    wild[0, 0], wild[T - 1, E - 1] = -2 ** 31, 2 ** 31 - 1
    assert (wild == -3).any() and (wild == 100).any() and not np.array_equal(np.clip(wild, 0, fs - 1), wild)
    ages[0, 0], ages[T - 1, E - 1] = 0, fs - 1
    assert np.array_equal(np.clip(wild, 0, fs - 1), ages)
    df, dn = _dev(frames), _dev(nxt)
    da, dw = torch.from_numpy(ages).to(DEV), torch.from_numpy(wild).to(DEV)
    every = torch.arange(n, dtype=torch.int64, device=DEV)
    for second, dsecond, mode in ((nxt, dn, "two stores"), (None, None, "single store")):
        obs, nob = _call(df, dsecond, da, every, fs)
        want_obs, want_next = FC.frames_reference(frames, second, ages, np.arange(n), fs)
        _assert_same(obs, want_obs, mode + " observations vs the numpy restatement")
        _assert_same(nob, want_next, mode + " next_observations vs the numpy restatement")
        wobs, wnob = _call(df, dsecond, dw, every, fs)
        assert not MG.differing([dict(obs), dict(nob)], [dict(wobs), dict(wnob)]), mode + ": ages outside [0, fs - 1] are not clamped"
        # rows -1 and T n_envs among valid ones
        rows = torch.tensor([3, -1, 0, n, n - 1, -2 ** 40, 2 ** 40, 5], dtype=torch.int64, device=DEV)
        bad = torch.tensor([False, True, False, True, False, True, True, False], device=DEV)
        good = torch.tensor([3, 0, n - 1, 5], dtype=torch.int64, device=DEV)
        got, want = _call(df, dsecond, dw, rows, fs), _call(df, dsecond, da, good, fs)
        for half, whalf in zip(got, want):
            for key in whalf:
                assert torch.isnan(half[key][bad]).all(), (mode, key)
                assert torch.equal(half[key][~bad], whalf[key]), (mode, key)
        for shift in range(n):
            got = _call(df, dsecond, da, every, fs, row_shift=shift)
            want = _call(df, dsecond, da, (every + shift) % n, fs)
            assert not MG.differing([dict(x) for x in got], [dict(x) for x in want]), f"{mode} row_shift={shift}"
    # a frame stack longer than the ring: every step is taken modulo T
    long_ages = torch.full((T, E), 11, dtype=torch.int32, device=DEV)
    obs, nob = _call(df, None, long_ages, every, 12)
    want_obs, want_next = FC.frames_reference(frames, None, long_ages.cpu().numpy(), np.arange(n), 12)
    _assert_same(obs, want_obs, "fs = 12 > T observations")
    _assert_same(nob, want_next, "fs = 12 > T next_observations")


def test_gather_load_frames_argument_rejections():
    frames, nxt, ages = _direct(2, (8, 8), (4, 4), 2, (U8, F32), seed=41)
    df, dn, da = _dev(frames), _dev(nxt), torch.from_numpy(ages).to(DEV)
    rows = torch.zeros(2, dtype=torch.int64, device=DEV)
    with pytest.raises(ValueError, match="ages must be a contiguous int32 tensor of shape"):
        P.gather_load_frames(df["image"], df["tactile"], da.to(torch.int64), rows, frame_stack=2)
    with pytest.raises(ValueError, match="ages must be a contiguous int32 tensor of shape"):
        P.gather_load_frames(df["image"], df["tactile"], da[:-1], rows, frame_stack=2)
    with pytest.raises(m3l_amd.M3LError, match="must live on the GPU"):
        P.gather_load_frames(df["image"], df["tactile"], da.cpu(), rows, frame_stack=2)
    with pytest.raises(ValueError, match="frame_stack=0"):
        P.gather_load_frames(df["image"], df["tactile"], da, rows, frame_stack=0)
    with pytest.raises(ValueError, match="image_next_frames must be a contiguous tensor of image_frames' shape and dtype"):
        P.gather_load_frames(df["image"], df["tactile"], da, rows, dn["image"][:-1], frame_stack=2)
    with pytest.raises(ValueError, match="tactile_next_frames must be"):
        P.gather_load_frames(df["image"], None, da, rows, None, dn["tactile"], frame_stack=2)
    with pytest.raises(ValueError, match=r"image_frames must be a contiguous uint8 / float32 \(T, n_envs, \.\.\.\) tensor of 5 dimensions"):
        P.gather_load_frames(df["image"][:, :, None], None, da, rows, frame_stack=2)
    with pytest.raises(ValueError, match="tactile_frames must be"):
        P.gather_load_frames(df["image"], df["tactile"][:-1], da, rows, frame_stack=2)
    with pytest.raises(ValueError, match="rows must be a contiguous 1-D int64 tensor"):
        P.gather_load_frames(df["image"], df["tactile"], da, rows.to(torch.int32), frame_stack=2)
    with pytest.raises(m3l_amd.M3LError, match="row_shift=14"):
        P.gather_load_frames(df["image"], df["tactile"], da, rows, row_shift=14, frame_stack=2)
    dbuf = _buffers(2, False, (8, 8), (4, 4), 2, (U8, F32), stacked=False)[1]
    obs = {"image": torch.zeros(E, 2, 8, 8, 3, dtype=torch.uint8), "tactile": torch.zeros(E, 2, 6, 4, 4)}
    with pytest.raises(ValueError, match="needs `done` there"):
        dbuf.add(obs, obs, np.zeros((E, A), F32), np.zeros(E, F32), torch.zeros(E, device=DEV), [{}] * E)
    assert dbuf.pos == 0


def test_gather_load_frames_64_bit_offsets():
    """Case 4.  A never-initialised float32 single frame store of 174800 slots of 64 x 64 x 3 = 12288 elements (8.6 GB): the last slots start
    beyond 2^31 elements.  Written and sampled: slot 0, whose stack reaches back across the wrap to the last two slots; the last slot, whose next
    frame is slot 0; and the slots round element 2^31."""
    Tb, fs, H, W = 174800, 3, 64, 64
    per = H * W * 3
    store = torch.empty(Tb, 1, H, W, 3, dtype=torch.float32, device=DEV)
    mid = 2 ** 31 // per
    assert store.numel() > 2 ** 31 and mid * per < 2 ** 31 < (mid + 1) * per and (Tb - 3) * per > 2 ** 31 and mid + 2 < Tb - 3
    sampled = [0, Tb - 1, mid + 1, mid]
    touched = sorted({(r + d) % Tb for r in sampled for d in (-2, -1, 0, 1)})
    g = np.random.default_rng(13)
    frames = dict(zip(touched, g.random((len(touched), H, W, 3), dtype=np.float32)))
    for s, f in frames.items():
        store[s, 0].copy_(torch.from_numpy(f))
    ages = torch.zeros(Tb, 1, dtype=torch.int32, device=DEV)
    ages[sampled] = fs - 1
    order = [1, 0, 3, 2, 1]
    rows = torch.tensor([sampled[o] for o in order], dtype=torch.int64, device=DEV)
    obs, nob = P.gather_load_frames(store, None, ages, rows, frame_stack=fs)
    for got, offsets, what in ((obs, (-2, -1, 0), "observations"), (nob, (-1, 0, 1), "next_observations")):
        stacks = np.stack([np.stack([frames[(sampled[o] + d) % Tb] for d in offsets]) for o in order])
        _assert_same(got, RC.vt_load_reference(RC.flatten_frame_stack({"image": stacks}), fs), what + " vs the numpy restatement of the written slots")


# ---- the buffer
def _filled(n_adds, fs, single, seed, hw=((8, 8), (4, 4)), dtypes=(U8, F32), **kw):
    st = FC.make_stream(n_adds, E, fs, hw[0], hw[1], 2, dtypes[0], dtypes[1], A, seed)
    sbuf, dbuf = _buffers(fs, single, hw[0], hw[1], 2, dtypes, **kw)
    for k in range(n_adds):
        _add(sbuf, st, k)
        _add(dbuf, st, k)
    return st, sbuf, dbuf


@pytest.mark.parametrize("single", [False, True], ids=["two_stores", "single_store"])
def test_drawn_rows_cover_the_valid_set_and_nothing_else(single):
    """Case 5.  4096 draws from a full T = 7, fs = 3 buffer with pos = 3: 5 valid steps of 2 environments with two stores, 4 with one.  A
    given pair is missed with probability 0.9^4096 with 10 valid pairs (0.875^4096 with 8)."""
    fs = 3
    st, sbuf, dbuf = _filled(17, fs, single, seed=51)
    _, model = FC.fill_models(17, T, fs, single, st)
    valid = model.valid_steps()
    assert valid == ([6, 0, 1, 2] if single else [5, 6, 0, 1, 2]) and dbuf.pos == 3
    torch.manual_seed(17)
    batch = dbuf.sample(4096)
    rows = batch.rows.cpu().numpy()
    assert batch.rows.dtype == torch.int64 and batch.rows.device == torch.device(DEV) and rows.shape == (4096,)
    assert set(rows.tolist()) == {t * E + e for t in valid for e in range(E)}
    # the batch is the one those rows name
    t, e = rows // E, rows % E
    _check_batch(batch, sbuf.sample(1, indices=(t, e)), t, e, 17, st, fs, single, ((0, 1), (-1, 1)), "drawn batch")
    assert batch.actions.shape == (4096, A) and batch.rewards.shape == (4096, 1) and batch.dones.shape == (4096, 1)


def test_two_calls_with_the_same_indices_give_equal_bits():
    """Case 10."""
    st, sbuf, dbuf = _filled(9, 4, False, seed=61)
    t, e = [5, 6, 0, 1, 1], [0, 1, 1, 0, 0]
    a, b = dbuf.sample(1, indices=(t, e)), dbuf.sample(1, indices=(np.array(t), torch.tensor(e)))
    assert not MG.differing(list(a), list(b))
    assert not torch.isnan(a.observations["image"]).any() and not torch.equal(a.observations["image"][0], a.observations["image"][1])


def test_memory_contract_of_gather_load_frames(monkeypatch):
    """Case 6.  Guards intact and equal bits under the 0xFF and 0x00 fills, at the shapes of cases 1 and 2 with B = 5, in both store modes."""
    cases = [(fs, (8, 8), (4, 4), 2, dt) for fs in (1, 2, 3, 4) for dt in ((U8, F32), (F32, F32), (F32, U8))]
    cases += [(3, (6, 10), (5, 3), 1, (U8, F32)), (3, (5, 5), (5, 3), 4, (F32, U8)), (3, (5, 5), (4, 4), 4, (U8, F32)), (3, (5, 5), None, 0, (U8, None)),
              (3, (8, 8), None, 0, (F32, None)), (3, None, (5, 3), 4, (None, F32)), (3, None, (4, 4), 1, (None, U8))]
    made = []
    for i, (fs, ihw, thw, S, dt) in enumerate(cases):
        frames, nxt, ages = _direct(fs, ihw, thw, S, dt, seed=300 + 2 * i)
        made.append((fs, _dev(frames), _dev(nxt), torch.from_numpy(ages).to(DEV)))
    rows = torch.tensor([0, T * E - 1, 2, 2, 0], dtype=torch.int64, device=DEV)

    def work(g):
        out = {}
        for i, (fs, df, dn, da) in enumerate(made):
            out[f"two{i}"] = [dict(x) for x in _call(df, dn, da, rows, fs)]
            out[f"one{i}"] = [dict(x) for x in _call(df, None, da, rows, fs, row_shift=i % (T * E))]
        g.check("after gather_load_frames")
        return out
    MG.run_contract(monkeypatch, work, need_ws=False)


@pytest.mark.parametrize("single", [False, True], ids=["two_stores", "single_store"])
def test_check_stacking(single):
    """Case 7.  The generated streams pass; each rule of the contract is named when it is broken, and a refused add() stores nothing."""
    for fs in (1, 2, 3, 4):
        st = FC.make_stream(17, E, fs, (8, 8), (4, 4), 2, U8, F32, A, seed=70 + fs)
        _, plain = _buffers(fs, single, (8, 8), (4, 4), 2, (U8, F32), stacked=False)
        _, checked = _buffers(fs, single, (8, 8), (4, 4), 2, (U8, F32), stacked=False, check_stacking=True)
        for k in range(17):
            _add(plain, st, k)
            _add(checked, st, k)
        first, count = checked._valid_steps()
        t, e = np.repeat([(first + u) % T for u in range(count)], E), np.tile(np.arange(E), count)
        assert not MG.differing(list(plain.sample(1, indices=(t, e))), list(checked.sample(1, indices=(t, e))))
    fs = 3
    st = FC.make_stream(6, E, fs, (8, 8), (4, 4), 2, U8, F32, A, seed=77, lengths=lambda fs_, e: [9])       # no episode ends within 6 adds
    assert not st["dones"].any()

    def fresh(n):
        buf = _buffers(fs, single, (8, 8), (4, 4), 2, (U8, F32), stacked=False, check_stacking=True)[1]
        for k in range(n):
            _add(buf, st, k)
        return buf

    def step(k, **changed):
        args = dict(obs={key: v[k].copy() for key, v in st["obs"].items()}, next_obs={key: v[k].copy() for key, v in st["next_obs"].items()})
        for name, (key, env, frame) in changed.items():
            args[name][key][env, frame] = args[name][key][env, frame] + 1
        return args["obs"], args["next_obs"], st["actions"][k], st["rewards"][k], st["dones"][k], st["infos"][k]

    buf = fresh(2)
    with pytest.raises(ValueError, match=r"observation 'tactile' of environment 1 .*next_obs\[:, :-1\] == obs\[:, 1:\]"):
        buf.add(*step(2, next_obs=("tactile", 1, 0)))
    with pytest.raises(ValueError, match=r"observation 'image' of environment 0 .*obs equals the previous add\(\)'s next_obs"):
        buf.add(*step(3))                                                  # add 2 was skipped: obs is not the previous next_obs
    assert buf.pos == 2 and buf._age.tolist() == [1, 1]
    buf.add(*step(2))                                                      # the refused adds changed nothing: the stream goes on
    assert buf.pos == 3 and buf._age.tolist() == [2, 2]
    with pytest.raises(ValueError, match=r"observation 'image' of environment 0 .*all frames of obs are equal at an episode's first step"):
        fresh(0).add(*step(2))                                             # a first add() whose stack is not constant
    buf = fresh(0)
    with pytest.raises(ValueError, match=r"observation 'tactile' of environment 1 .*all frames of obs are equal"):
        buf.add(*step(0, obs=("tactile", 1, 0)))                           # the oldest frame alone differs: next_obs[:, :-1] == obs[:, 1:] holds
    assert buf.pos == 0
    # after a done the next stack must be constant again
    ends = FC.make_stream(3, E, fs, (8, 8), (4, 4), 2, U8, F32, A, seed=78, lengths=lambda fs_, e: [2 + e])
    buf = _buffers(fs, single, (8, 8), (4, 4), 2, (U8, F32), stacked=False, check_stacking=True)[1]
    for k in range(2):
        _add(buf, ends, k)
    assert ends["dones"][1].tolist() == [True, False] and ends["ages"][2].tolist() == [0, 2]
    obs = {key: v[2].copy() for key, v in ends["obs"].items()}
    obs["image"][0] = ends["next_obs"]["image"][1, 0]                      # environment 0 goes on as if its episode had not ended
    nxt = {key: v[2].copy() for key, v in ends["next_obs"].items()}
    nxt["image"][0, :-1] = obs["image"][0, 1:]
    with pytest.raises(ValueError, match=r"observation 'image' of environment 0 .*all frames of obs are equal"):
        buf.add(obs, nxt, ends["actions"][2], ends["rewards"][2], ends["dones"][2], ends["infos"][2])
    _add(buf, ends, 2)
    assert buf.pos == 3


def test_the_references_default_buffer_fits():
    """Case 8.  10^6 transitions at the reference's shapes (frame_stack 4, image 64 x 64 x 3 uint8, two tactile sensors 32 x 32 x 3 float32):
    arithmetic only, nothing is allocated.  A stacked store that does not fit names frame_dedup=True among the ways out."""
    shapes = {"image": (4, 64, 64, 3), "tactile": (4, 6, 32, 32)}
    dts = {"image": U8, "tactile": F32}
    before = torch.cuda.memory_allocated(DEV)
    two = m3l_amd.DeviceReplayBuffer(1_000_000, 1, shapes, dts, 7, frame_dedup=True, device=DEV)
    assert two.store_bytes()["total"] == 73_772_000_000 == 2 * 36864 * 10 ** 6 + 4 * 10 ** 6 * 10 + 4 * 10 ** 6
    one = m3l_amd.DeviceReplayBuffer(1_000_000, 1, shapes, dts, 7, optimize_memory_usage=True, handle_timeout_termination=False, frame_dedup=True,
                                     device=DEV)
    assert one.store_bytes()["total"] == 36_864_000_000 + 4 * 10 ** 6 * 9 + 4 * 10 ** 6
    assert two.store_bytes()["total"] < torch.cuda.mem_get_info(DEV)[1]               # it fits the card, with room for the model
    buf = m3l_amd.DeviceReplayBuffer(4_000_000, 1, shapes, dts, 7, device=DEV)
    obs = {"image": np.zeros((1,) + shapes["image"], U8), "tactile": np.zeros((1,) + shapes["tactile"], F32)}
    with pytest.raises(m3l_amd.M3LError) as err:
        buf.add(obs, obs, np.zeros((1, 7), F32), np.zeros(1, F32), np.zeros(1, bool), [{}])
    msg = str(err.value)
    for way in ("uint8", "optimize_memory_usage=True", "smaller buffer_size", "frame_dedup=True"):
        assert way in msg
    assert f"{4 * 73_772_000_000} B" in msg and "295.1 GB" in msg
    assert len(re.findall(r"(\d+) bytes", msg)) == 2                                   # need and free, as before
    assert buf.observations is None and buf.frames is None and torch.cuda.memory_allocated(DEV) == before
    # a deduplicated buffer that does not fit names the three ways it has left
    huge = m3l_amd.DeviceReplayBuffer(40_000_000, 1, shapes, dts, 7, frame_dedup=True, device=DEV)
    with pytest.raises(m3l_amd.M3LError) as err:
        huge.add(obs, obs, np.zeros((1, 7), F32), np.zeros(1, F32), np.zeros(1, bool), [{}])
    assert "frame_dedup" not in str(err.value) and "smaller buffer_size" in str(err.value) and huge.frames is None


def test_buffer_end_to_end():
    """Case 9.  fs = 2, image 32 x 32, tactile 16 x 16: MAEExtractor on the deduplicated batch's observations and next observations computes the
    bits it computes on the stacked buffer's batch."""
    from m3l_amd import VTMAE, VTT, MAEExtractor
    fs, S = 2, 2
    st, sbuf, dbuf = _filled(9, fs, False, seed=81, hw=((32, 32), (16, 16)))
    t, e = np.array([1, 0, 6, 4, 1, 3]), np.array([0, 1, 0, 1, 1, 0])
    batch, ref = dbuf.sample(6, indices=(t, e)), sbuf.sample(6, indices=(t, e))
    _check_batch(batch, ref, t, e, 9, st, fs, False, ((0, 1), (-1, 1)), "end to end")
    torch.manual_seed(3)
    enc = VTT(image_size=32, tactile_size=16, image_patch_size=8, tactile_patch_size=4, dim=64, depth=2, heads=2, mlp_dim=128,
              image_channels=3 * fs, tactile_channels=3 * fs, num_tactiles=S, frame_stack=fs)
    mae = VTMAE(encoder=enc, decoder_dim=64, masking_ratio=0.75, decoder_depth=1, decoder_heads=2, num_tactiles=S, frame_stack=fs)
    ext = MAEExtractor(mae, 64, vision_only_control=False, frame_stack=fs).to(DEV)
    with torch.no_grad():
        f, f_next = ext(batch.observations), ext(batch.next_observations)
        assert f.shape == (6, 64) and torch.equal(f, ext(ref.observations)) and torch.equal(f_next, ext(ref.next_observations))
        assert not torch.equal(f, f_next) and torch.isfinite(f).all()
