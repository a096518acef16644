"""The device-resident rollout on a real MI355X (csrc/rollout.hip, m3l_amd/rollout.py).

Gather-and-load is held to equal bits three ways: the reference's recorded minibatches (golden/rollout_feed.npz), the numpy restatement
of tests/rollout_cases.py, and today's composed path on a device-resident store — index_select on the reference-ordered store ->
fusion._flatten_frame_stack -> vt_load.  Shapes are the smallest that reach every path of the kernel: pixel counts that are and are not a
multiple of the 4-element vector (image 8x8 and 6x10 vs 5x5; tactile 3*4*4 = 48 vs 3*5*3 = 45), widths that are no multiple of it, T != n_envs
(an un-swapped index map fails), one to four sensors, one block and several.  GAE is held to the float64 restatement within 1e-4 of the largest
absolute entry, the bound of the head tests (expected fp32 error: a few ulp / (1 - gamma lambda), about 1e-5 relative)."""
import os

import numpy as np
import pytest
import torch

import memguard as MG
import rollout_cases as RC

pytestmark = pytest.mark.gpu

import m3l_amd  # noqa: E402
from m3l_amd import rollout as R  # noqa: E402
from m3l_amd import vt_load  # noqa: E402
from m3l_amd.fusion import _flatten_frame_stack  # noqa: E402

DEV = "cuda:0"
T, E = 3, 2
U8, F32 = np.uint8, np.float32


def _dev(stores):
    return {k: torch.from_numpy(v).to(DEV) for k, v in stores.items()}


def _composed(dstores, idx, fs, img_range=(0, 1), tac_range=(-1, 1), rows=None):
    """Today's ops on a resident store: the reference-ordered (swapped, flattened) store, index_select, the frame-stack flatten, vt_load.
    rows: store rows taken directly instead (the 64-bit test, where the swapped copy of the store would be another 4.4 GB)."""
    picked = {}
    for k, v in dstores.items():
        if rows is None:
            picked[k] = v.transpose(0, 1).reshape((-1,) + tuple(v.shape[2:])).index_select(0, idx)
        else:
            picked[k] = v.reshape((-1,) + tuple(v.shape[2:])).index_select(0, rows)
    return vt_load(_flatten_frame_stack(picked), image_normalization=list(img_range), tactile_normalization=list(tac_range), frame_stack=fs, device=DEV)


def _assert_same(got, want, what):
    assert sorted(got) == sorted(want), what
    for k in want:
        w = want[k] if isinstance(want[k], torch.Tensor) else torch.from_numpy(np.ascontiguousarray(want[k])).to(DEV)
        assert got[k].dtype == torch.float32 and got[k].is_cuda and got[k].shape == w.shape, (what, k)
        assert torch.equal(got[k], w), f"{what}: {k} differs in {(got[k] != w).sum().item()} of {w.numel()} elements"


def _index_lists(n):
    g = np.random.default_rng(n)
    return {1: [n - 1], 5: [0, n - 1, 2, 2, 0], 64: [0, n - 1] + g.integers(0, n, 62).tolist()}


def _check_case(stores, fs, img_range=(0, 1), tac_range=(-1, 1)):
    ds = _dev(stores)
    for B, idx in _index_lists(T * E).items():
        assert len(idx) == B
        di = torch.tensor(idx, dtype=torch.int64, device=DEV)
        got = R.gather_load(ds.get("image"), ds.get("tactile"), di, img_range, tac_range)
        assert isinstance(got, R.LoadedObs)
        _assert_same(got, RC.feed_reference(stores, idx, img_range, tac_range), f"B={B} vs the numpy restatement")
        _assert_same(got, _composed(ds, di, fs, img_range, tac_range), f"B={B} vs index_select -> flatten -> vt_load")


@pytest.mark.parametrize("variant", sorted(RC.GOLDEN_VARIANTS))
def test_gather_load_matches_the_reference_minibatches(golden_dir, variant):
    z = np.load(os.path.join(golden_dir, "rollout_feed.npz"))
    _, _, img_range, tac_range = RC.GOLDEN_VARIANTS[variant]
    ds = _dev({k: z[f"{variant}/store/{k}"] for k in ("image", "tactile")})
    rows = [torch.from_numpy(z[f"{variant}/store/{k}"]).to(DEV) for k in ("actions", "values", "log_probs", "advantages", "returns")]
    for i in range(len(RC.GOLDEN_INDEX_LISTS)):
        idx = torch.from_numpy(z[f"{variant}/idx{i}"]).to(DEV)
        got = R.gather_load(ds["image"], ds["tactile"], idx, img_range, tac_range)
        _assert_same(got, {k: z[f"{variant}/out{i}/x/{k}"] for k in ("image", "tactile1", "tactile2")}, f"{variant} list {i}")
        got = R.gather_rows(*rows, idx)
        for t, k in zip(got, ("actions", "old_values", "old_log_prob", "advantages", "returns")):
            assert torch.equal(t.cpu(), torch.from_numpy(z[f"{variant}/out{i}/{k}"])), (variant, i, k)


@pytest.mark.parametrize("image_hw,tactile_hw", [((8, 8), (4, 4)), ((6, 10), (5, 3))], ids=["8x8_4x4", "6x10_5x3"])
@pytest.mark.parametrize("S", [1, 2, 4])
@pytest.mark.parametrize("fs", [1, 2])
@pytest.mark.parametrize("dtypes", [(U8, F32), (F32, F32), (F32, U8)], ids=["u8_f32", "f32_f32", "f32_u8"])
def test_gather_load_bit_equal_to_composed_path(dtypes, fs, S, image_hw, tactile_hw):
    _check_case(RC.make_stores(T, E, fs, image_hw, tactile_hw, S, dtypes[0], dtypes[1], seed=fs * 100 + S * 10 + image_hw[0]), fs)


@pytest.mark.parametrize("dtype", [U8, F32], ids=["u8", "f32"])
def test_gather_load_element_wise_image_path(dtype):
    """5 x 5 = 25 pixels: no multiple of 4, so the image moves element by element (and 3 * 5 * 3 = 45 tactile elements likewise)."""
    _check_case(RC.make_stores(T, E, 2, (5, 5), (5, 3), 2, dtype, dtype, seed=55), 2)


@pytest.mark.parametrize("dtype", [U8, F32], ids=["u8", "f32"])
def test_gather_load_image_only_and_tactile_only(dtype):
    _check_case(RC.make_stores(T, E, 2, (8, 8), None, 0, dtype, None, seed=61), 2)
    _check_case(RC.make_stores(T, E, 2, None, (4, 4), 2, None, dtype, seed=62), 2)
    _check_case(RC.make_stores(T, E, 1, (6, 10), None, 0, dtype, None, seed=63), 1)
    _check_case(RC.make_stores(T, E, 1, None, (5, 3), 4, None, dtype, seed=64), 1)


def test_gather_load_non_default_ranges():
    """[0, 255] / [-2, 3] on uint8 frames (vt_load_u8.npz) and [0.1, 0.3] / [-0.7, 0.9], which binary floats cannot represent (vt_load_frac.npz):
    the span is formed in double and rounded once."""
    _check_case(RC.make_stores(T, E, 2, (8, 8), (4, 4), 2, U8, U8, seed=71), 2, (0, 255), (-2, 3))
    _check_case(RC.make_stores(T, E, 2, (6, 10), (5, 3), 2, U8, F32, seed=72), 2, (0, 255), (-2, 3))
    _check_case(RC.make_stores(T, E, 1, (8, 8), (4, 4), 2, F32, F32, seed=73), 1, (0.1, 0.3), (-0.7, 0.9))
    _check_case(RC.make_stores(T, E, 2, (5, 5), (5, 3), 1, F32, F32, seed=74), 2, (0.1, 0.3), (-0.7, 0.9))


def test_gather_load_64_bit_offsets():
    """A uint8 image store of 90000 rows of 4 x 64 x 64 x 3 bytes = 4.4 GB, never initialised: rows on both sides of byte offsets 2^31 and
    2^32 (and the first and last row) are written and sampled."""
    Tb, Eb, fs, H, W = 45000, 2, 4, 64, 64
    row_bytes = fs * H * W * 3
    store = torch.empty(Tb, Eb, fs, H, W, 3, dtype=torch.uint8, device=DEV)
    assert store.numel() > 2 ** 32
    rows = [0, 2 ** 31 // row_bytes - 1, 2 ** 31 // row_bytes, 2 ** 31 // row_bytes + 1, 2 ** 32 // row_bytes - 1, 2 ** 32 // row_bytes,
            2 ** 32 // row_bytes + 1, Tb * Eb - 1]
    assert rows[2] * row_bytes < 2 ** 31 < (rows[2] + 1) * row_bytes and rows[5] * row_bytes < 2 ** 32 < (rows[5] + 1) * row_bytes
    g = np.random.default_rng(9)
    frames = g.integers(0, 256, (len(rows), fs, H, W, 3), dtype=np.uint8)
    flat = store.view(Tb * Eb, fs, H, W, 3)
    for r, f in zip(rows, frames):
        flat[r].copy_(torch.from_numpy(f))
    idx = [(r % Eb) * Tb + r // Eb for r in rows]                   # row = t * n_envs + env  <-  flat index env * T + t
    order = [3, 0, 7, 5, 1, 6, 2, 4, 3]
    di = torch.tensor([idx[o] for o in order], dtype=torch.int64, device=DEV)
    got = R.gather_load(store, None, di, (0, 255))
    want = RC.vt_load_reference(RC.flatten_frame_stack({"image": frames[order]}), fs, (0, 255))
    _assert_same(got, want, "vs the numpy restatement of the written rows")
    drows = torch.tensor([rows[o] for o in order], dtype=torch.int64, device=DEV)
    _assert_same(got, _composed({"image": store}, None, fs, (0, 255), rows=drows), "vs index_select -> flatten -> vt_load on those rows")


def _scalars(Tn, En, A, seed, **kw):
    sc = RC.make_scalars(Tn, En, A, seed, **kw)
    return sc, {k: torch.from_numpy(v).to(DEV) for k, v in sc.items()}


@pytest.mark.parametrize("A", [1, 7])
@pytest.mark.parametrize("B", [1, 5])
def test_gather_rows_bit_equal_to_index_select(A, B):
    sc, d = _scalars(T, E, A, 80 + A)
    adv, ret = R.gae(d["rewards"], d["values"], d["episode_starts"], d["last_values"], d["dones"], 0.99, 0.95)
    src = [d["actions"], d["values"], d["log_probs"], adv, ret]
    idx = torch.tensor(_index_lists(T * E)[B], dtype=torch.int64, device=DEV)
    got = R.gather_rows(*src, idx)
    assert got[0].shape == (B, A) and all(t.shape == (B,) for t in got[1:])
    for g, s in zip(got, src):
        want = s.transpose(0, 1).reshape((T * E,) + tuple(s.shape[2:])).index_select(0, idx)
        assert torch.equal(g, want)


@pytest.mark.parametrize("gamma,lam", [(0.99, 0.95), (1.0, 1.0)])
@pytest.mark.parametrize("En", [1, 3])
@pytest.mark.parametrize("Tn", [1, 5])
def test_gae_against_float64(Tn, En, gamma, lam):
    sc, d = _scalars(Tn, En, 1, 90 + Tn + En)
    assert sc["dones"].any() and (Tn < 3 or sc["episode_starts"][1:].any())
    args = (d["rewards"], d["values"], d["episode_starts"], d["last_values"], d["dones"], gamma, lam)
    adv, ret = R.gae(*args)
    adv2, ret2 = R.gae(*args)
    assert torch.equal(adv, adv2) and torch.equal(ret, ret2)
    want_adv, want_ret = RC.gae_reference(sc["rewards"], sc["values"], sc["episode_starts"], sc["last_values"], sc["dones"], gamma, lam)
    for name, got, want in (("advantages", adv, want_adv), ("returns", ret, want_ret)):
        err = np.abs(got.cpu().numpy().astype(np.float64) - want).max()
        print(f"gae T={Tn} n_envs={En} gamma={gamma} lambda={lam} {name}: max error {err:.3e}, largest entry {np.abs(want).max():.3e}")
        assert err <= 1e-4 * np.abs(want).max(), (name, err)


def test_memory_contract_of_the_three_entry_points(monkeypatch):
    """Guards intact and equal bits under the 0xFF and 0x00 fills, at the shapes of the bit-equality cases with B = 5."""
    cases = [(dt, fs, S, ihw, thw) for dt in ((U8, F32), (F32, U8)) for fs in (1, 2) for S in (1, 2, 4) for ihw, thw in (((8, 8), (4, 4)), ((6, 10), (5, 3)))]
    cases += [((U8, U8), 2, 2, (5, 5), (5, 3)), ((F32, F32), 2, 2, (8, 8), None), ((F32, F32), 2, 4, None, (5, 3))]
    stores = [(_dev(RC.make_stores(T, E, fs, ihw, thw, S, dt[0], dt[1], seed=i)), fs) for i, (dt, fs, S, ihw, thw) in enumerate(cases)]
    idx = torch.tensor(_index_lists(T * E)[5], dtype=torch.int64, device=DEV)
    scal = [_scalars(T, E, A, 120 + A)[1] for A in (1, 7)]

    def work(g):
        out = {}
        for i, (ds, fs) in enumerate(stores):
            out[f"load{i}"] = dict(R.gather_load(ds.get("image"), ds.get("tactile"), idx))
        g.check("after gather_load")
        for i, d in enumerate(scal):
            adv, ret = R.gae(d["rewards"], d["values"], d["episode_starts"], d["last_values"], d["dones"], 0.99, 0.95)
            g.check("after gae")
            out[f"gae{i}"] = [adv, ret]
            out[f"rows{i}"] = list(R.gather_rows(d["actions"], d["values"], d["log_probs"], adv, ret, idx))
            g.check("after gather_rows")
        return out
    MG.run_contract(monkeypatch, work, need_ws=False)


def test_buffer_end_to_end():
    """add() over T = 3 steps -> get(batch_size=4, indices) yields 4 and 2 rows whose x is the gather-and-load of those rows, and MAEExtractor on
    that x computes the bits it computes on the raw observations of the same rows."""
    from m3l_amd import VTMAE, VTT, MAEExtractor
    fs, S, A = 2, 2, 3
    stores = RC.make_stores(T, E, fs, (32, 32), (16, 16), S, U8, F32, seed=130)
    sc = RC.make_scalars(T, E, A, 131)
    buf = m3l_amd.DeviceRolloutBuffer(T, E, {"image": (fs, 32, 32, 3), "tactile": (fs, 3 * S, 16, 16)}, {"image": U8, "tactile": F32}, A, device=DEV)
    for t in range(T):
        assert (buf.pos, buf.full) == (t, False)
        buf.add({k: v[t] for k, v in stores.items()}, sc["actions"][t], sc["rewards"][t], sc["episode_starts"][t],
                torch.from_numpy(sc["values"][t]).to(DEV)[:, None], torch.from_numpy(sc["log_probs"][t]).to(DEV))
    assert buf.full and buf.pos == T
    buf.compute_returns_and_advantage(torch.from_numpy(sc["last_values"]).to(DEV), sc["dones"].astype(bool))
    want_adv, want_ret = RC.gae_reference(sc["rewards"], sc["values"], sc["episode_starts"], sc["last_values"], sc["dones"], 0.99, 0.95)
    assert np.abs(buf.advantages.cpu().numpy() - want_adv).max() <= 1e-4 * np.abs(want_adv).max()
    indices = [4, 0, 5, 2, 2, 1]
    batches = list(buf.get(batch_size=4, indices=indices))
    assert [b.actions.shape[0] for b in batches] == [4, 2]
    ds = _dev(stores)
    per_step = {"actions": sc["actions"], "old_values": sc["values"], "old_log_prob": sc["log_probs"], "advantages": buf.advantages.cpu().numpy(),
                "returns": buf.returns.cpu().numpy()}
    torch.manual_seed(3)
    enc = VTT(image_size=32, tactile_size=16, image_patch_size=8, tactile_patch_size=4, dim=64, depth=2, heads=2, mlp_dim=128,
              image_channels=3 * fs, tactile_channels=3 * fs, num_tactiles=S, frame_stack=fs)
    mae = VTMAE(encoder=enc, decoder_dim=64, masking_ratio=0.75, decoder_depth=1, decoder_heads=2, num_tactiles=S, frame_stack=fs)
    ext = MAEExtractor(mae, 64, vision_only_control=False, frame_stack=fs).to(DEV)
    for b, idx in zip(batches, (indices[:4], indices[4:])):
        assert isinstance(b.x, m3l_amd.LoadedObs) and b.observations is b.x
        di = torch.tensor(idx, dtype=torch.int64, device=DEV)
        _assert_same(b.x, R.gather_load(ds["image"], ds["tactile"], di), "batch.x vs gather_load")
        _assert_same(b.x, RC.feed_reference(stores, idx), "batch.x vs the numpy restatement")
        for k, v in per_step.items():
            want = RC.swap_and_flatten(v)[np.asarray(idx)]
            assert torch.equal(getattr(b, k).cpu(), torch.from_numpy(want if k == "actions" else want.reshape(-1))), k
        # the raw observations of the same rows take the extractor's own path: frame-stack flatten -> vt_load with the default ranges
        raw = {k: torch.from_numpy(RC.swap_and_flatten(v)[np.asarray(idx)]).to(DEV) for k, v in stores.items()}
        with torch.no_grad():
            f_loaded = ext(b.x)
            f_raw = ext(raw)
        assert f_loaded.shape == (len(idx), 64) and torch.equal(f_loaded, f_raw)
    # a permutation drawn on the device covers every row once; the last batch is short
    sizes, seen = [], []
    for b in buf.get(batch_size=4):
        sizes.append(b.actions.shape[0])
        seen.append(b.old_values)
    assert sizes == [4, 2]
    assert torch.equal(torch.cat(seen).sort().values, buf.values.flatten().sort().values)
    buf.reset()
    assert (buf.pos, buf.full) == (0, False)
