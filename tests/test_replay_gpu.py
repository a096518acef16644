"""The device-resident replay buffer on a real MI355X (csrc/replay.hip, m3l_amd/replay.py).

`observations` and `next_observations` are held to equal bits three ways, in both store modes (a second store; the single store's next slot):
the numpy restatement of tests/replay_cases.py, today's composed path on a device-resident store — index_select -> fusion._flatten_frame_stack
-> vt_load — and, for `observations`, the reference's recorded minibatches (golden/rollout_feed.npz).  Shapes are the rollout tests', the smallest
that reach every path of the kernel: pixel counts that are and are not a multiple of the 4-element vector (image 8x8 and 6x10 vs 5x5; tactile
3*4*4 = 48 vs 3*5*3 = 45), T = 3 != n_envs = 2 (a transposed row map fails), one to four sensors, one block and several.  The scalars are
copies and 0 / 1 products (equal bits); the normalised rewards are one IEEE division by a scale rounded once (equal bits against numpy's
float32, 2^-22 relative against float64: two roundings of 2^-24 each with a factor 2 of margin)."""
import os
import re
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import memguard as MG
import replay_cases as PC
import rollout_cases as RC

pytestmark = pytest.mark.gpu

import m3l_amd  # noqa: E402
from m3l_amd import replay as P  # noqa: E402
from m3l_amd import vt_load  # noqa: E402
from m3l_amd.fusion import _flatten_frame_stack  # noqa: E402

DEV = "cuda:0"
T, E = 3, 2
U8, F32 = np.uint8, np.float32


def _dev(stores):
    return None if stores is None else {k: torch.from_numpy(np.ascontiguousarray(v)).to(DEV) for k, v in stores.items()}


def _composed(dstores, rows, fs, img_range=(0, 1), tac_range=(-1, 1)):
    """Today's ops on a resident store: index_select of the store's rows, the frame-stack flatten, vt_load."""
    picked = {k: v.reshape((-1,) + tuple(v.shape[2:])).index_select(0, rows) for k, v in dstores.items()}
    return vt_load(_flatten_frame_stack(picked), image_normalization=list(img_range), tactile_normalization=list(tac_range), frame_stack=fs, device=DEV)


def _assert_same(got, want, what):
    assert sorted(got) == sorted(want), what
    for k in want:
        w = want[k] if isinstance(want[k], torch.Tensor) else torch.from_numpy(np.ascontiguousarray(want[k])).to(DEV)
        assert got[k].dtype == torch.float32 and got[k].is_cuda and got[k].shape == w.shape, (what, k)
        assert torch.equal(got[k], w), f"{what}: {k} differs in {(got[k] != w).sum().item()} of {w.numel()} elements"


def _row_lists(n):
    """B = 1 / 5 / 64 with repeated, first and last rows; the last row is of step T - 1, whose single-store next observation wraps to step 0."""
    g = np.random.default_rng(n)
    return {1: [n - 1], 5: [0, n - 1, 2, 2, 0], 64: [0, n - 1] + g.integers(0, n, 62).tolist()}


def _next_rows(rows, Tn, En):
    rows = np.asarray(rows)
    return ((rows // En + 1) % Tn) * En + rows % En


def _check_case(stores, fs, img_range=(0, 1), tac_range=(-1, 1), seed=0):
    """Both store modes against the numpy restatement and the composed device path, for every row list."""
    kinds = {k: v.dtype for k, v in stores.items()}
    g = np.random.default_rng(1000 + seed)
    # a second store of other seeded frames: reading the first store, or the next slot of either, cannot pass for it
    second = {k: (g.integers(0, 256, v.shape, dtype=np.uint8) if kinds[k] == U8 else (2 * g.random(v.shape, dtype=np.float32) - 1).astype(np.float32))
              for k, v in stores.items()}
    ds, dn = _dev(stores), _dev(second)
    for nxt, dnxt, mode in ((second, dn, "two stores"), (None, None, "single store")):
        for B, rows in _row_lists(T * E).items():
            assert len(rows) == B
            dr = torch.tensor(rows, dtype=torch.int64, device=DEV)
            obs, nobs = P.gather_load(ds.get("image"), ds.get("tactile"), dr, None if dnxt is None else dnxt.get("image"),
                                      None if dnxt is None else dnxt.get("tactile"), img_range, tac_range)
            assert isinstance(obs, m3l_amd.LoadedObs) and isinstance(nobs, m3l_amd.LoadedObs)
            t, e = np.asarray(rows) // E, np.asarray(rows) % E
            want = PC.sample_reference(stores, nxt, dict(actions=np.zeros((T, E, 1), F32), rewards=np.zeros((T, E), F32), dones=np.zeros((T, E), F32)),
                                       t, e, T, None, img_range, tac_range)
            _assert_same(obs, want["observations"], f"{mode} B={B} observations vs the numpy restatement")
            _assert_same(nobs, want["next_observations"], f"{mode} B={B} next_observations vs the numpy restatement")
            _assert_same(obs, _composed(ds, dr, fs, img_range, tac_range), f"{mode} B={B} observations vs index_select -> flatten -> vt_load")
            if dnxt is None:
                dnr = torch.tensor(_next_rows(rows, T, E), dtype=torch.int64, device=DEV)
                _assert_same(nobs, _composed(ds, dnr, fs, img_range, tac_range), f"{mode} B={B} next_observations vs the composed path")
            else:
                _assert_same(nobs, _composed(dnxt, dr, fs, img_range, tac_range), f"{mode} B={B} next_observations vs the composed path")


@pytest.mark.parametrize("variant", sorted(RC.GOLDEN_VARIANTS))
def test_gather_load_matches_the_reference_minibatches(golden_dir, variant):
    """The recorded minibatches of the reference's own run: flat index j of its swapped order is row (j % T) * n_envs + j // T here."""
    z = np.load(os.path.join(golden_dir, "rollout_feed.npz"))
    _, _, img_range, tac_range = RC.GOLDEN_VARIANTS[variant]
    stores = {k: z[f"{variant}/store/{k}"] for k in ("image", "tactile")}
    ds = _dev(stores)
    dn = {k: torch.roll(v, -1, 0).contiguous() for k, v in ds.items()}       # the second store holds what the single store's next slot holds
    for i in range(len(RC.GOLDEN_INDEX_LISTS)):
        j = z[f"{variant}/idx{i}"]
        rows = torch.from_numpy((j % T) * E + j // T).to(DEV)
        want = {k: z[f"{variant}/out{i}/x/{k}"] for k in ("image", "tactile1", "tactile2")}
        want_next = RC.feed_reference(stores, (j // T) * T + (j % T + 1) % T, img_range, tac_range)
        for nxt in (dn, None):
            obs, nobs = P.gather_load(ds["image"], ds["tactile"], rows, nxt and nxt["image"], nxt and nxt["tactile"], img_range, tac_range)
            _assert_same(obs, want, f"{variant} list {i} observations")
            _assert_same(nobs, want_next, f"{variant} list {i} next_observations")


@pytest.mark.parametrize("image_hw,tactile_hw", [((8, 8), (4, 4)), ((6, 10), (5, 3))], ids=["8x8_4x4", "6x10_5x3"])
@pytest.mark.parametrize("S", [1, 2, 4])
@pytest.mark.parametrize("fs", [1, 2])
@pytest.mark.parametrize("dtypes", [(U8, F32), (F32, F32), (F32, U8)], ids=["u8_f32", "f32_f32", "f32_u8"])
def test_gather_load_bit_equal_to_composed_path(dtypes, fs, S, image_hw, tactile_hw):
    seed = fs * 100 + S * 10 + image_hw[0]
    _check_case(RC.make_stores(T, E, fs, image_hw, tactile_hw, S, dtypes[0], dtypes[1], seed=seed), fs, seed=seed)


@pytest.mark.parametrize("dtype", [U8, F32], ids=["u8", "f32"])
def test_gather_load_element_wise_paths(dtype):
    """5 x 5 = 25 pixels: no multiple of 4, so the image moves element by element (and 3 * 5 * 3 = 45 tactile elements likewise)."""
    _check_case(RC.make_stores(T, E, 2, (5, 5), (5, 3), 2, dtype, dtype, seed=55), 2, seed=55)


@pytest.mark.parametrize("dtype", [U8, F32], ids=["u8", "f32"])
def test_gather_load_image_only_and_tactile_only(dtype):
    _check_case(RC.make_stores(T, E, 2, (8, 8), None, 0, dtype, None, seed=61), 2, seed=61)
    _check_case(RC.make_stores(T, E, 2, None, (4, 4), 2, None, dtype, seed=62), 2, seed=62)
    _check_case(RC.make_stores(T, E, 1, (6, 10), None, 0, dtype, None, seed=63), 1, seed=63)
    _check_case(RC.make_stores(T, E, 1, None, (5, 3), 4, None, dtype, seed=64), 1, seed=64)


def test_gather_load_non_default_ranges():
    """[0, 255] / [-2, 3] on uint8 frames and [0.1, 0.3] / [-0.7, 0.9], which binary floats cannot represent: the span is formed in double and
    rounded once."""
    _check_case(RC.make_stores(T, E, 2, (8, 8), (4, 4), 2, U8, U8, seed=71), 2, (0, 255), (-2, 3), seed=71)
    _check_case(RC.make_stores(T, E, 2, (6, 10), (5, 3), 2, U8, F32, seed=72), 2, (0, 255), (-2, 3), seed=72)
    _check_case(RC.make_stores(T, E, 1, (8, 8), (4, 4), 2, F32, F32, seed=73), 1, (0.1, 0.3), (-0.7, 0.9), seed=73)
    _check_case(RC.make_stores(T, E, 2, (5, 5), (5, 3), 1, F32, F32, seed=74), 2, (0.1, 0.3), (-0.7, 0.9), seed=74)


def test_single_store_wrap_and_row_shift():
    """A row of step T - 1 takes its next observation from step 0 of the same environment; row_shift moves every row round the ring."""
    stores = RC.make_stores(T, E, 2, (8, 8), (4, 4), 2, U8, F32, seed=81)
    ds = _dev(stores)
    last = torch.tensor([(T - 1) * E + e for e in range(E)], dtype=torch.int64, device=DEV)
    first = torch.tensor(list(range(E)), dtype=torch.int64, device=DEV)
    _, nobs = P.gather_load(ds["image"], ds["tactile"], last)
    obs0, _ = P.gather_load(ds["image"], ds["tactile"], first)
    _assert_same(nobs, dict(obs0), "next observation of step T - 1 vs the observation of step 0")
    assert not torch.equal(nobs["image"][0], nobs["image"][1])                      # the two environments' frames differ
    every = torch.arange(T * E, dtype=torch.int64, device=DEV)
    for shift in (0, 1, E, T * E - 1):
        obs, nobs = P.gather_load(ds["image"], ds["tactile"], every, row_shift=shift)
        moved = (every + shift) % (T * E)
        want, want_next = P.gather_load(ds["image"], ds["tactile"], moved)
        _assert_same(obs, dict(want), f"row_shift={shift} observations")
        _assert_same(nobs, dict(want_next), f"row_shift={shift} next_observations")
        rows_out = P.gather_rows(torch.zeros(T, E, 1, device=DEV), torch.zeros(T, E, device=DEV), torch.zeros(T, E, device=DEV), None, every,
                                 row_shift=shift, return_rows=True)[3]
        assert rows_out.dtype == torch.int64 and torch.equal(rows_out, moved)


def test_gather_load_64_bit_offsets():
    """A never-initialised uint8 single store of 45000 x 2 rows of 4 x 64 x 64 x 3 = 49152 bytes (4.4 GB): rows on both sides of byte offsets
    2^31 and 2^32, the first row, and a row of the last step whose next observation wraps to step 0; those rows and their next rows are written,
    then sampled."""
    Tb, Eb, fs, H, W = 45000, 2, 4, 64, 64
    row_bytes = fs * H * W * 3
    store = torch.empty(Tb, Eb, fs, H, W, 3, dtype=torch.uint8, device=DEV)
    assert store.numel() > 2 ** 32
    rows = [0, 2 ** 31 // row_bytes - 1, 2 ** 31 // row_bytes, 2 ** 31 // row_bytes + 1, 2 ** 32 // row_bytes - 1, 2 ** 32 // row_bytes,
            2 ** 32 // row_bytes + 1, Tb * Eb - 1]
    assert rows[2] * row_bytes < 2 ** 31 < (rows[2] + 1) * row_bytes and rows[5] * row_bytes < 2 ** 32 < (rows[5] + 1) * row_bytes
    nrows = _next_rows(rows, Tb, Eb).tolist()
    assert nrows[-1] == Eb - 1 and nrows[0] == Eb                                    # the last step wraps to step 0
    touched = sorted(set(rows) | set(nrows))
    g = np.random.default_rng(9)
    frames = dict(zip(touched, g.integers(0, 256, (len(touched), fs, H, W, 3), dtype=np.uint8)))
    flat = store.view(Tb * Eb, fs, H, W, 3)
    for r, f in frames.items():
        flat[r].copy_(torch.from_numpy(f))
    order = [3, 0, 7, 5, 1, 6, 2, 4, 3]
    dr = torch.tensor([rows[o] for o in order], dtype=torch.int64, device=DEV)
    obs, nobs = P.gather_load(store, None, dr, image_normalization=(0, 255))
    for got, pick, what in ((obs, rows, "observations"), (nobs, nrows, "next_observations")):
        want = RC.vt_load_reference(RC.flatten_frame_stack({"image": np.stack([frames[pick[o]] for o in order])}), fs, (0, 255))
        _assert_same(got, want, f"{what} vs the numpy restatement of the written rows")
        drows = torch.tensor([pick[o] for o in order], dtype=torch.int64, device=DEV)
        _assert_same(got, _composed({"image": store}, drows, fs, (0, 255)), f"{what} vs index_select -> flatten -> vt_load on those rows")


# ---- scalars
def _scalars(A, seed):
    sc = PC.make_replay_scalars(T, E, A, seed)
    return sc, {k: torch.from_numpy(v).to(DEV) for k, v in sc.items()}


def _flat(t):
    return t.reshape((T * E,) + tuple(t.shape[2:]))


@pytest.mark.parametrize("A", [1, 7])
@pytest.mark.parametrize("B", [1, 5, 64])
def test_gather_rows_bit_equal_to_index_select(A, B):
    sc, d = _scalars(A, 80 + A)
    rows = _row_lists(T * E)[B]
    dr = torch.tensor(rows, dtype=torch.int64, device=DEV)
    actions, rewards, dones = P.gather_rows(d["actions"], d["rewards"], d["dones"], d["timeouts"], dr)
    assert actions.shape == (B, A) and rewards.shape == (B, 1) and dones.shape == (B, 1)
    assert torch.equal(actions, _flat(d["actions"]).index_select(0, dr))
    assert torch.equal(rewards[:, 0], _flat(d["rewards"]).index_select(0, dr))
    masked = (_flat(d["dones"]) * (1 - _flat(d["timeouts"]))).index_select(0, dr)
    assert torch.equal(dones[:, 0], masked)
    # rows 0 and T n_envs - 1 are in every list with B > 1: a done that was a truncation is masked, a true termination is kept
    fd, ft = sc["dones"].reshape(-1), sc["timeouts"].reshape(-1)
    if B > 1:
        assert any(fd[r] == 1 and ft[r] == 1 for r in rows) and any(fd[r] == 1 and ft[r] == 0 for r in rows)
        assert dones[rows.index(0), 0] == 0 and dones[rows.index(T * E - 1), 0] == 1
    else:
        assert fd[rows[0]] == 1 and ft[rows[0]] == 0 and dones[0, 0] == 1
    # without timeout handling the dones come out as stored
    _, _, plain = P.gather_rows(d["actions"], d["rewards"], d["dones"], None, dr)
    assert torch.equal(plain[:, 0], _flat(d["dones"]).index_select(0, dr)) and (B == 1 or not torch.equal(plain, dones))
    want = PC.sample_reference({"image": np.zeros((T, E, 1, 1, 1, 3), U8)}, None, sc, np.asarray(rows) // E, np.asarray(rows) % E, T)
    for got, k in ((actions, "actions"), (rewards, "rewards"), (dones, "dones")):
        assert torch.equal(got.cpu(), torch.from_numpy(want[k])), k


@pytest.mark.parametrize("A", [1, 7])
@pytest.mark.parametrize("return_rows", [False, True])
def test_gather_rows_out_of_range_rows(A, return_rows):
    """Rows -1 and T n_envs among B = 5: NaN in the three float outputs and -1 in `rows`, every entry in range bit-equal to index_select.  The
    kernel's `rows` output is optional: with and without it."""
    _, d = _scalars(A, 80 + A)
    rows = [0, -1, T * E - 1, T * E, 2]
    dr = torch.tensor(rows, dtype=torch.int64, device=DEV)
    got = P.gather_rows(d["actions"], d["rewards"], d["dones"], d["timeouts"], dr, return_rows=return_rows)
    assert len(got) == 3 + return_rows
    actions, rewards, dones = got[:3]
    assert actions.shape == (5, A) and rewards.shape == (5, 1) and dones.shape == (5, 1)
    bad = torch.tensor([r < 0 or r >= T * E for r in rows], device=DEV)
    assert bad.sum() == 2
    ok = dr[~bad]
    assert torch.isnan(actions[bad]).all() and torch.isnan(rewards[bad]).all() and torch.isnan(dones[bad]).all()
    assert torch.equal(actions[~bad], _flat(d["actions"]).index_select(0, ok))
    assert torch.equal(rewards[~bad, 0], _flat(d["rewards"]).index_select(0, ok))
    assert torch.equal(dones[~bad, 0], (_flat(d["dones"]) * (1 - _flat(d["timeouts"]))).index_select(0, ok))
    if return_rows:
        assert got[3].dtype == torch.int64 and got[3].tolist() == [0, -1, T * E - 1, -1, 2]


def test_normalised_rewards():
    sc, d = _scalars(2, 91)
    var, eps, clip = 3.7, 1e-8, 1.25
    env = SimpleNamespace(norm_obs=False, norm_reward=True, ret_rms=SimpleNamespace(var=np.float64(var)), epsilon=eps, clip_reward=clip)
    scale, c = P.reward_normalization(env)
    dr = torch.arange(T * E, dtype=torch.int64, device=DEV)
    got = P.gather_rows(d["actions"], d["rewards"], d["dones"], d["timeouts"], dr, scale, c)[1].cpu().numpy()[:, 0]
    want32 = PC.normalize_reward_reference(sc["rewards"].reshape(-1), var, eps, clip)
    want64 = PC.normalize_reward_reference(sc["rewards"].reshape(-1), var, eps, clip, dtype=np.float64)
    rel = np.abs(got.astype(np.float64) - want64) / np.abs(want64)
    print(f"normalised rewards: max relative error against float64 {rel.max():.3e} (bound {2.0 ** -22:.3e}); values {got.tolist()}")
    np.testing.assert_array_equal(got, want32)
    assert np.all(rel <= 2.0 ** -22)
    assert (got == np.float32(clip)).any() and (got == np.float32(-clip)).any() and (np.abs(got) < np.float32(clip)).any()


# ---- the buffer
SMALL = dict(fs=2, image_hw=(8, 8), tactile_hw=(4, 4), S=2, A=3)


def _filled(n_adds, single_store, seed, handle_timeouts=None, hw=None, dtypes=(U8, F32)):
    """A T = 3, n_envs = 2 buffer after n_adds adds of seeded steps, the numpy stores a host replay buffer would hold after the same adds (built
    from the pure-Python ring model), and the model.  In the single-store mode step k's next observation is step k + 1's observation, as an
    environment without resets yields them (the mode assumes it); with two stores the next observations are frames of their own."""
    fs, S, A = SMALL["fs"], SMALL["S"], SMALL["A"]
    ihw, thw = hw or (SMALL["image_hw"], SMALL["tactile_hw"])
    handle_timeouts = (not single_store) if handle_timeouts is None else handle_timeouts
    seq = RC.make_stores(n_adds + 1, E, fs, ihw, thw, S, dtypes[0], dtypes[1], seed)           # seq[k]: what the env shows before step k
    other = RC.make_stores(n_adds, E, fs, ihw, thw, S, dtypes[0], dtypes[1], seed + 1)
    nxt = {k: v[1:] for k, v in seq.items()} if single_store else other
    g = np.random.default_rng(seed + 2)
    steps = dict(actions=g.standard_normal((n_adds, E, A)).astype(F32), rewards=(3 * g.standard_normal((n_adds, E))).astype(F32),
                 dones=(g.random((n_adds, E)) < 0.5), timeouts=np.zeros((n_adds, E), bool))
    steps["dones"][-1, 0] = steps["timeouts"][-1, 0] = True                                    # a truncation among the newest steps
    steps["dones"][-1, 1], steps["timeouts"][-1, 1] = True, False                              # and a true termination
    buf = m3l_amd.DeviceReplayBuffer(T * E, E, {"image": (fs,) + ihw + (3,), "tactile": (fs, 3 * S) + thw}, {"image": dtypes[0], "tactile": dtypes[1]}, A,
                                     optimize_memory_usage=single_store, handle_timeout_termination=handle_timeouts, device=DEV)
    assert buf.buffer_size == T
    model = PC.RingModel(T, single_store)
    for k in range(n_adds):
        infos = [{"TimeLimit.truncated": True} if steps["timeouts"][k, e] else {} for e in range(E)]
        buf.add({key: v[k] for key, v in seq.items()}, {key: v[k] for key, v in nxt.items()}, steps["actions"][k], steps["rewards"][k], steps["dones"][k], infos)
        model.add()
        assert (buf.pos, buf.full, buf.size()) == (model.pos, model.full, model.size())
    held = lambda tag, key: (seq if tag[0] == "obs" else nxt)[key][tag[1]]      # noqa: E731
    stores = {key: np.stack([held(model.obs[t], key) if model.obs[t] else np.zeros_like(seq[key][0]) for t in range(T)]) for key in seq}
    nstores = None if single_store else {key: np.stack([held(model.next_obs[t], key) if model.next_obs[t] else np.zeros_like(seq[key][0])
                                                        for t in range(T)]) for key in seq}
    ks = [model.step[t] if model.step[t] is not None else 0 for t in range(T)]
    scalars = dict(actions=steps["actions"][ks], rewards=steps["rewards"][ks], dones=steps["dones"][ks].astype(F32),
                   timeouts=steps["timeouts"][ks].astype(F32) if handle_timeouts else None)
    return buf, model, stores, nstores, scalars


def _assert_batch(batch, want, what):
    assert isinstance(batch, m3l_amd.ReplayBatch)
    _assert_same(batch.observations, want["observations"], what + " observations")
    _assert_same(batch.next_observations, want["next_observations"], what + " next_observations")
    for k in ("actions", "dones", "rewards", "rows"):
        got = getattr(batch, k)
        assert got.is_cuda and torch.equal(got.cpu(), torch.from_numpy(np.ascontiguousarray(want[k]))), (what, k)


@pytest.mark.parametrize("single_store", [False, True], ids=["two_stores", "single_store"])
def test_ring_overwrites_and_injected_indices(single_store):
    """5 adds at T = 3: slots 0 and 1 return the overwriting steps' data; in the single-store mode the slot after the newest step holds that
    step's next observation.  Two calls with the same indices give equal bits."""
    buf, model, stores, nstores, scalars = _filled(5, single_store, seed=140)
    assert (buf.pos, buf.full) == (2, True) and model.step == [3, 4, 2]
    valid = model.valid_steps()
    assert valid == ([0, 1] if single_store else [0, 1, 2])
    t = np.array([s for s in valid for _ in range(E)] + [valid[-1]])
    e = np.array([x for _ in valid for x in range(E)] + [0])
    batch = buf.sample(99, indices=(t, e))
    want = PC.sample_reference(stores, nstores, scalars, t, e, T)
    _assert_batch(batch, want, "after 5 adds")
    again = buf.sample(99, indices=(t.tolist(), torch.from_numpy(e)))
    assert not MG.differing(list(batch), list(again))
    if single_store:
        assert model.next_of(1) == ("next", 4) and model.obs[2] == ("next", 4)
        with pytest.raises(ValueError, match="indices"):
            buf.sample(1, indices=([2], [0]))                                       # step pos: overwritten by the newest next observation
    else:
        # the newest steps carry a truncation (env 0) and a termination (env 1): masked and kept
        i0, i1 = (int(np.flatnonzero((t == 1) & (e == x))[0]) for x in (0, 1))
        assert scalars["dones"][1, 0] == 1 and scalars["timeouts"][1, 0] == 1 and batch.dones[i0, 0] == 0
        assert scalars["dones"][1, 1] == 1 and scalars["timeouts"][1, 1] == 0 and batch.dones[i1, 0] == 1
    with pytest.raises(ValueError, match="norm_obs"):
        buf.sample(4, env=SimpleNamespace(norm_obs=True, norm_reward=True))
    # reward normalisation through the buffer; norm_reward false leaves them raw
    env = SimpleNamespace(norm_obs=False, norm_reward=True, ret_rms=SimpleNamespace(var=2.5), epsilon=1e-8, clip_reward=1.0)
    _assert_batch(buf.sample(99, env=env, indices=(t, e)), PC.sample_reference(stores, nstores, scalars, t, e, T, (2.5, 1e-8, 1.0)), "normalised")
    env.norm_reward = False
    _assert_batch(buf.sample(99, env=env, indices=(t, e)), want, "norm_reward false")


def test_timeout_handling_off_leaves_dones_unmasked():
    buf, model, stores, nstores, scalars = _filled(3, False, seed=150, handle_timeouts=False)
    assert buf.timeouts is None and scalars["timeouts"] is None and (buf.pos, buf.full) == (0, True)
    t, e = np.array([2, 2, 0, 1]), np.array([0, 1, 1, 0])
    batch = buf.sample(4, indices=(t, e))
    _assert_batch(batch, PC.sample_reference(stores, nstores, scalars, t, e, T), "handle_timeout_termination=False")
    assert batch.dones[0, 0] == 1 and batch.dones[1, 0] == 1                        # the truncated step's done is not masked


@pytest.mark.parametrize("n_adds,single_store,valid", [(5, True, [0, 1]), (4, True, [2, 0]), (2, True, [0, 1]), (2, False, [0, 1]), (5, False, [0, 1, 2])],
                         ids=["single_full_pos2", "single_full_pos1", "single_part", "two_part", "two_full"])
def test_drawn_rows_cover_the_valid_set_and_nothing_else(n_adds, single_store, valid):
    """4096 draws over at most 6 valid (t, e) pairs: a given pair is missed with probability at most (5 / 6)^4096 (0.75^4096 with 4 pairs)."""
    buf, model, stores, nstores, scalars = _filled(n_adds, single_store, seed=160 + n_adds)
    assert model.valid_steps() == valid and (not (single_store and buf.full) or buf.pos not in valid)
    torch.manual_seed(n_adds)
    batch = buf.sample(4096)
    rows = batch.rows.cpu().numpy()
    assert batch.rows.dtype == torch.int64 and batch.rows.device == torch.device(DEV) and rows.shape == (4096,)
    assert set(rows.tolist()) == {t * E + e for t in valid for e in range(E)}
    # the batch is the one those rows name
    _assert_batch(batch, PC.sample_reference(stores, nstores, scalars, rows // E, rows % E, T), "drawn batch")
    assert batch.actions.shape == (4096, SMALL["A"]) and batch.rewards.shape == (4096, 1) and batch.dones.shape == (4096, 1)


def test_stores_that_do_not_fit_are_refused_before_any_allocation():
    """4 x 10^6 transitions at the reference's shapes: 1.18 TB in two stores, four times the card's 288 GiB (SB3's default of 10^6 is 295 GB, which
    leaves no room for anything else)."""
    shapes = {"image": (4, 64, 64, 3), "tactile": (4, 6, 32, 32)}
    buf = m3l_amd.DeviceReplayBuffer(4_000_000, 1, shapes, {"image": U8, "tactile": F32}, 7, device=DEV)
    obs = {"image": np.zeros((1,) + shapes["image"], U8), "tactile": np.zeros((1,) + shapes["tactile"], F32)}
    before = torch.cuda.memory_allocated(DEV)
    with pytest.raises(m3l_amd.M3LError) as err:
        buf.add(obs, obs, np.zeros((1, 7), F32), np.zeros(1, F32), np.zeros(1, bool), [{}])
    msg = str(err.value)
    need, free = (int(x) for x in re.findall(r"(\d+) bytes", msg))                   # both numbers are named
    assert need == buf.store_bytes()["total"] == 4 * 294_952_000_000
    assert 0 < free <= torch.cuda.mem_get_info(DEV)[1] < need
    for way in ("uint8", "optimize_memory_usage=True", "smaller buffer_size"):
        assert way in msg
    assert buf.observations is None and buf.pos == 0 and torch.cuda.memory_allocated(DEV) == before


def test_memory_contract_of_both_entry_points(monkeypatch):
    """Guards intact and equal bits under the 0xFF and 0x00 fills, at the shapes of the bit-equality cases with B = 5, in both store modes."""
    cases = [(dt, fs, S, ihw, thw) for dt in ((U8, F32), (F32, U8)) for fs in (1, 2) for S in (1, 2, 4) for ihw, thw in (((8, 8), (4, 4)), ((6, 10), (5, 3)))]
    cases += [((U8, U8), 2, 2, (5, 5), (5, 3)), ((F32, F32), 2, 2, (8, 8), None), ((F32, F32), 2, 4, None, (5, 3))]
    stores = [(_dev(RC.make_stores(T, E, fs, ihw, thw, S, dt[0], dt[1], seed=i)), _dev(RC.make_stores(T, E, fs, ihw, thw, S, dt[0], dt[1], seed=500 + i)))
              for i, (dt, fs, S, ihw, thw) in enumerate(cases)]
    rows = torch.tensor(_row_lists(T * E)[5], dtype=torch.int64, device=DEV)
    scal = [_scalars(A, 120 + A)[1] for A in (1, 7)]

    def work(g):
        out = {}
        for i, (ds, dn) in enumerate(stores):
            out[f"two{i}"] = [dict(x) for x in P.gather_load(ds.get("image"), ds.get("tactile"), rows, dn.get("image"), dn.get("tactile"))]
            out[f"one{i}"] = [dict(x) for x in P.gather_load(ds.get("image"), ds.get("tactile"), rows, row_shift=i % (T * E))]
        g.check("after gather_load")
        for i, d in enumerate(scal):
            out[f"rows{i}"] = list(P.gather_rows(d["actions"], d["rewards"], d["dones"], d["timeouts"], rows, 1.5, 2.0, row_shift=1, return_rows=True))
            out[f"raw{i}"] = list(P.gather_rows(d["actions"], d["rewards"], d["dones"], None, rows))
            g.check("after gather_rows")
        return out
    MG.run_contract(monkeypatch, work, need_ws=False)


def test_buffer_end_to_end():
    """add() for 5 steps into T = 3 with infos carrying a truncation -> sample(indices): MAEExtractor on the batch's observations and next
    observations computes the bits it computes on the raw rows, and SACHead.td_target on the batch's (B, 1) rewards and dones equals the call
    with the composed (B,) vectors."""
    from m3l_amd import VTMAE, VTT, MAEExtractor, SACHead
    fs, S, A = SMALL["fs"], SMALL["S"], SMALL["A"]
    buf, model, stores, nstores, scalars = _filled(5, False, seed=170, hw=((32, 32), (16, 16)))
    t, e = np.array([1, 0, 2, 1, 1, 0]), np.array([0, 1, 0, 1, 0, 0])
    env = SimpleNamespace(norm_obs=False, norm_reward=True, ret_rms=SimpleNamespace(var=1.7), epsilon=1e-8, clip_reward=2.0)
    batch = buf.sample(6, env=env, indices=(t, e))
    want = PC.sample_reference(stores, nstores, scalars, t, e, T, (1.7, 1e-8, 2.0))
    _assert_batch(batch, want, "end to end")
    assert scalars["timeouts"][1, 0] == 1 and batch.dones[0, 0] == 0 and batch.dones[3, 0] == 1
    torch.manual_seed(3)
    enc = VTT(image_size=32, tactile_size=16, image_patch_size=8, tactile_patch_size=4, dim=64, depth=2, heads=2, mlp_dim=128,
              image_channels=3 * fs, tactile_channels=3 * fs, num_tactiles=S, frame_stack=fs)
    mae = VTMAE(encoder=enc, decoder_dim=64, masking_ratio=0.75, decoder_depth=1, decoder_heads=2, num_tactiles=S, frame_stack=fs)
    ext = MAEExtractor(mae, 64, vision_only_control=False, frame_stack=fs).to(DEV)
    head = SACHead(64, A, net_arch=dict(pi=[32], qf=[32])).to(DEV)
    raw = {k: torch.from_numpy(v[t, e]).to(DEV) for k, v in stores.items()}
    raw_next = {k: torch.from_numpy(v[t, e]).to(DEV) for k, v in nstores.items()}
    with torch.no_grad():
        f, f_next = ext(batch.observations), ext(batch.next_observations)
        assert f.shape == (6, 64) and torch.equal(f, ext(raw)) and torch.equal(f_next, ext(raw_next))
        assert not torch.equal(f, f_next)
        noise = torch.randn(6, A, generator=torch.Generator().manual_seed(5)).to(DEV)
        composed_r = torch.from_numpy(want["rewards"][:, 0].copy()).to(DEV)
        composed_d = (torch.from_numpy(scalars["dones"][t, e]) * (1 - torch.from_numpy(scalars["timeouts"][t, e]))).to(DEV)
        tq = head.td_target(f_next, batch.rewards, batch.dones, 0.99, ent_coef=0.2, noise=noise)
        assert tq.shape == (6,) and torch.equal(tq, head.td_target(f_next, composed_r, composed_d, 0.99, ent_coef=0.2, noise=noise))
