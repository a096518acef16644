"""CPU-only checks of prioritised replay (DeviceReplayBuffer(prioritized=True), m3l_replay_per_refresh / _add / _sample / _update,
m3l_sac_critic_loss_w_fwd): the float64 restatement of tests/per_cases.py against cases written out by hand, the coverage conditions of the
inputs that test_replay_per_gpu.py runs, the rejections of the constructor, of the functional forms and of the entry points before any
launch, and the ABI.  No kernel is launched here."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import m3l_amd
import per_cases as PC
from m3l_amd import _lib as L
from m3l_amd import replay as P
from m3l_amd import sac as S

NEW_SYMBOLS = ("m3l_replay_per_refresh", "m3l_replay_per_add", "m3l_replay_per_sample", "m3l_replay_per_update", "m3l_sac_critic_loss_w_fwd")
F32 = np.float32
B_ = PC.PER_BLOCK


def _header():
    return open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "m3l_amd.h")).read()


def _declared(hdr, name):
    m = re.search(r"\bint " + name + r"\(([^)]*)\)", hdr)
    assert m, name
    return [" ".join(p.split()) for p in m.group(1).split(",")]


def _ctype_of(param):
    if "*" in param:
        return C.c_void_p
    return {"int": C.c_int, "long": C.c_long, "float": C.c_float, "double": C.c_double}[param.split()[0]]


def test_exports_and_abi():
    assert L.lib().m3l_version() >= 415
    hdr = _header()
    assert "prioritised replay (ABI 415)" in hdr
    for name in NEW_SYMBOLS:
        assert name in L.EXPORTS and hasattr(L.lib(), name)
        res, args = L._SIGS[name]
        params = _declared(hdr, name)
        assert res is C.c_int and len(args) == len(params), (name, len(args), len(params))
        for a, p in zip(args, params):
            assert a is _ctype_of(p), (name, p, a)
    assert _declared(hdr, "m3l_replay_per_sample") == [
        "const float* mass", "const float* block_mass", "const float* block_min", "long N", "const float* u", "const int64_t* rows_in", "int B",
        "float beta", "int stratified", "int64_t* rows", "float* weights", "void* stream"]
    assert _declared(hdr, "m3l_replay_per_update") == [
        "float* mass", "float* block_mass", "float* block_min", "float* max_priority", "long N", "const int64_t* rows", "const float* td", "int B",
        "float alpha", "float priority_eps", "void* stream"]
    plain, weighted = _declared(hdr, "m3l_sac_critic_loss_fwd"), _declared(hdr, "m3l_sac_critic_loss_w_fwd")
    assert weighted == plain[:2] + ["const float* weights"] + plain[2:5] + ["float* td_abs", "void* stream"]
    for macro, value in (("M3L_PER_BLOCK", P.PER_BLOCK), ("M3L_PER_MAX_UPDATE", P.PER_MAX_UPDATE)):
        assert re.search(rf"#define {macro} {value}\b", hdr), macro
    assert int(re.search(r"#define M3L_PER_MAX_BLOCKS (\d+)", hdr).group(1)) * P.PER_BLOCK == P.PER_MAX_ROWS >= 2 ** 21
    for name in ("PrioritizedReplayBatch", "per_refresh", "per_sample", "per_update"):
        assert name in m3l_amd.__all__ and hasattr(m3l_amd, name)
    assert m3l_amd.PrioritizedReplayBatch._fields == m3l_amd.NStepReplayBatch._fields + ("weights",)
    for text in (P.__doc__, open(os.path.join(os.path.dirname(_header.__code__.co_filename), "..", "README.md")).read()):
        assert "parity unpinned" in text and "HER and prioritised sampling" not in text and "HER, prioritised sampling" not in text


# ---- the restatement against cases written out by hand
def test_five_rows_by_hand():
    """mass 2 0 0 5 1: prefix 2 2 2 7 8, total 8, B = 4 -> strata of width 2."""
    m = np.array([2, 0, 0, 5, 1], dtype=F32)
    u = np.array([0.0, 0.0, 0.5, 0.5], dtype=F32)
    ref = PC.sample_reference(m, u, 1.0)
    assert ref["x"].tolist() == [0.0, 2.0, 5.0, 7.0] and ref["total"] == 8.0
    # x = 2 lies exactly on the prefix of row 0 and of the zero run behind it: the first prefix that exceeds it is row 3's; x = 7 likewise -> row 4
    assert ref["rows"].tolist() == [0, 3, 3, 4]
    assert ref["weights"].ravel().tolist() == [0.5, 0.2, 0.2, 1.0]
    assert PC.sample_reference(m, u, 0.0)["weights"].ravel().tolist() == [1.0] * 4
    flat = PC.sample_reference(m, np.array([0.0, 0.25, 0.875, 0.99], dtype=F32), 0.5, stratified=False)
    assert flat["x"][:3].tolist() == [0.0, 2.0, 7.0] and flat["rows"].tolist() == [0, 3, 4, 4]
    np.testing.assert_allclose(flat["weights"].ravel(), [0.5 ** 0.5, 0.2 ** 0.5, 1.0, 1.0])
    # a target at or past the total (rounding could produce one): the last row of positive mass
    assert PC.flat_row(np.array([3, 0, 1, 0], dtype=F32), 4.0) == 2 and PC.flat_row(np.array([3, 0, 1, 0], dtype=F32), 3.0) == 2


def test_two_levels_by_hand():
    """Three blocks: 4 at the last leaf of block 0, block 1 empty, 4 at leaf 2 of block 2 behind two zeros, 8 at its last leaf."""
    m = np.zeros(3 * B_, dtype=F32)
    m[B_ - 1], m[2 * B_ + 2], m[3 * B_ - 1] = 4, 4, 8
    bm, bmin = PC.refresh_reference(m)
    assert bm.tolist() == [4.0, 0.0, 12.0] and bmin.tolist() == [4.0, np.inf, 4.0]
    u = np.array([0.0, 0.0, 0.5, 0.0], dtype=F32)               # x = 0, 4, 10, 12 with total / B = 4
    ref = PC.sample_reference(m, u, 1.0)
    assert ref["x"].tolist() == [0.0, 4.0, 10.0, 12.0]
    # x = 4 is the prefix of block 0 and of the empty block 1: block 2, residual 0, its first positive leaf; x = 8 would be the boundary to the last
    assert ref["rows"].tolist() == [B_ - 1, 2 * B_ + 2, 3 * B_ - 1, 3 * B_ - 1]
    assert [PC.flat_row(m, x) for x in (0.0, 3.999, 4.0, 7.999, 8.0, 15.9, 16.0)] == [B_ - 1, B_ - 1, 2 * B_ + 2, 2 * B_ + 2, 3 * B_ - 1, 3 * B_ - 1, 3 * B_ - 1]
    assert ref["weights"].ravel().tolist() == [1.0, 1.0, 0.5, 0.5]


def test_update_by_hand():
    m = np.array([1, 0, 2, 3, 1], dtype=F32)
    rows = [2, 2, 1, -1, 5, 3, 4, 2]
    td = np.array([0.5, -3.0, 9.0, 9.0, 9.0, np.nan, np.inf, 1.0], dtype=F32)
    eps = F32(0.25)
    got, mp, written = PC.update_reference(m, 2.0, rows, td, 0.5, eps)
    # row 2: the largest of 0.75, 3.25, 1.25; row 1 (zero mass), -1 and 5 skipped with their td of 9; rows 3 and 4 take the old max_priority 2
    assert written == [2, 3, 4] and mp == F32(3.25)
    np.testing.assert_allclose(got, [1, 0, 3.25 ** 0.5, 2 ** 0.5, 2 ** 0.5])
    got, mp, _ = PC.update_reference(m, 8.0, [0], np.array([1.0], dtype=F32), 1.0, eps)
    assert got[0] == 1.25 and mp == F32(8.0)                     # max_priority never decreases


# ---- the coverage conditions of the GPU test's inputs
def test_exact_cases_are_exact_and_hit_the_boundaries():
    cases = PC.exact_cases()
    sizes = {m.size for m, _ in cases.values()}
    assert sizes == {3 * B_ + 5, 5, PC.N_MANY} and PC.blocks_of(PC.N_MANY) > 256      # the issue's two sizes, and one with chunks of two blocks
    for name, (m, u) in cases.items():
        B = u.size
        total = float(m.astype(np.float64).sum())
        assert m.dtype == F32 and (m == np.round(m)).all() and m.min() >= 0 and m.max() <= 8, name
        assert B & (B - 1) == 0 and total % B == 0 and (u * 256 == np.round(u * 256)).all() and (u == 0).any() and u.max() < 1, name
        # every float32 operation of the path is exact: k + u has 16 bits, times the integer total / B < 2^8; all sums are integers < 2^24
        assert total < 2 ** 24 and total / B < 2 ** 8 and B <= 2 ** 8, name
        x = PC.targets(total, u)
        assert (x.astype(F32).astype(np.float64) == x).all(), name
        ref = PC.sample_reference(m, u, 0.5)
        assert ref["rows"].tolist() == [PC.flat_row(m, xk) for xk in x], name
    m, u = cases["zero_block_in_the_middle"]
    leaf_hits, block_hits = PC.boundary_hits(m, u)
    bm, _ = PC.refresh_reference(m)
    assert bm[1] == 0 and bm[0] > 0 and bm[2] > 0 and bm[3] > 0 and leaf_hits >= 10 and block_hits >= 1
    # the target on the end of block 0 and of the zero block: its row is the first positive leaf of block 2, behind the zero run at its head
    ref = PC.sample_reference(m, u, 0.5)
    k = int(np.flatnonzero(ref["x"] == bm[0])[0])
    r = int(ref["rows"][k])
    assert r >= 2 * B_ + 9 and m[r] > 0 and m[2 * B_:r].sum() == 0 and m[B_ - 7:B_].sum() == 0
    assert (m[3 * B_ - 3:3 * B_ + 2] == 0).all() and ref["rows"].max() == m.size - 1
    m, u = cases["sparse"]
    assert PC.boundary_hits(m, u)[1] >= 2 and PC.sample_reference(m, u, 0.5)["rows"].max() == m.size - 1
    m, u = cases["many_blocks"]
    bm, _ = PC.refresh_reference(m)
    ref = PC.sample_reference(m, u, 0.5)
    assert bm[100] == bm[101] == 0 and PC.boundary_hits(m, u)[1] >= 3 and ref["rows"].max() == m.size - 1
    k = int(np.flatnonzero(ref["x"] == np.cumsum(bm)[99])[0])
    assert ref["rows"][k] >= 102 * B_ and m[100 * B_:ref["rows"][k]].sum() == 0
    for name in ("big", "small"):
        m, u = cases[f"all_mass_in_the_last_leaf_{name}"]
        assert set(PC.sample_reference(m, u, 0.5)["rows"].tolist()) == {m.size - 1}
        m, u = cases[f"all_mass_in_the_first_leaf_{name}"]
        assert set(PC.sample_reference(m, u, 0.5)["rows"].tolist()) == {0}


def test_general_masses_meet_their_conditions():
    for n in (3 * B_ + 5, 5):
        m = PC.general_mass(n, seed=n)
        pos = m[m > 0]
        assert m.dtype == F32 and (m == 0).any() and pos.max() / pos.min() >= 0.99e6
        if n > B_:
            assert (m[B_ - 20:B_ + 30] == 0).all()


# ---- rejections: the constructor, the functional forms, the entry points
SHAPES = {"image": (2, 8, 8, 3), "tactile": (2, 6, 4, 4)}
DTYPES = {"image": np.uint8, "tactile": np.float32}


def _buffer(**kw):
    args = dict(buffer_size=14, n_envs=2, obs_shapes=SHAPES, obs_dtypes=DTYPES, action_dim=3)
    args.update(kw)
    return m3l_amd.DeviceReplayBuffer(**args)


def test_constructor():
    buf = _buffer()
    assert buf.prioritized is False and buf.mass is None and buf.block_mass is None and buf.max_priority is None
    plain = buf.store_bytes()["scalars"]
    buf = _buffer(prioritized=True)
    assert (buf.prioritized, buf.alpha, buf.beta, buf.priority_eps) == (True, 0.6, 0.4, 1e-6)
    assert buf.store_bytes()["scalars"] == plain + 4 * (14 + 2 * 1 + 1)
    for kw in (dict(frame_dedup=True), dict(n_steps=3), dict(frame_dedup=True, n_steps=3), dict(optimize_memory_usage=True, handle_timeout_termination=False),
               dict(optimize_memory_usage=True, handle_timeout_termination=False, frame_dedup=True)):
        assert _buffer(prioritized=True, alpha=0.0, beta=1.0, priority_eps=np.float32(0.5), **kw).prioritized
    for name in ("alpha", "beta"):
        for bad in (-0.1, 1.5, float("nan"), "0.5", None, True):
            with pytest.raises(ValueError, match=name + r"=.* must be a number in \[0, 1\]"):
                _buffer(prioritized=True, **{name: bad})
    for bad in (0.0, -1e-6, float("inf"), float("nan"), "1e-6", None):
        with pytest.raises(ValueError, match=r"priority_eps=.* must be a positive finite number"):
            _buffer(prioritized=True, priority_eps=bad)
    big = dict(obs_shapes={"image": (1, 2, 2, 3)}, obs_dtypes={"image": np.uint8})
    assert _buffer(buffer_size=2 ** 21, prioritized=True, **big).store_bytes()["scalars"] > 0
    assert _buffer(buffer_size=P.PER_MAX_ROWS, prioritized=True, **big).buffer_size == P.PER_MAX_ROWS // 2
    with pytest.raises(ValueError, match=rf"prioritized=True holds at most {P.PER_MAX_ROWS} transitions"):
        _buffer(buffer_size=P.PER_MAX_ROWS + 2, prioritized=True, **big)
    assert _buffer(buffer_size=P.PER_MAX_ROWS + 2, **big).prioritized is False
    with pytest.raises(ValueError, match="built without prioritized=True"):
        _buffer().update_priorities(torch.zeros(2, dtype=torch.int64), torch.zeros(2))


def test_functional_forms_refuse_host_tensors_and_bad_arguments():
    mass, blocks, one = torch.zeros(5), torch.zeros(1), torch.ones(1)
    rows, u = torch.zeros(2, dtype=torch.int64), torch.zeros(2)
    with pytest.raises(m3l_amd.M3LError, match="must live on the GPU"):
        P.per_refresh(mass)
    with pytest.raises(m3l_amd.M3LError, match="must live on the GPU"):
        P.per_sample(mass, blocks, blocks, u)
    with pytest.raises(m3l_amd.M3LError, match="must live on the GPU"):
        P.per_update(mass, blocks, blocks, one, rows, u)
    with pytest.raises(m3l_amd.M3LError, match="must live on the GPU"):
        S.critic_loss_from(torch.zeros(2, 3), torch.zeros(3), weights=torch.ones(3))


def test_entry_points_refuse_bad_arguments():
    lib = L.lib()
    p = 1 << 20

    def sample(mass=p, bm=p, bmin=p, N=5, u=p, rows_in=None, B=4, beta=0.4, strat=1, rows=p, w=p):
        return lib.m3l_replay_per_sample(mass, bm, bmin, N, u, rows_in, B, beta, strat, rows, w, None)

    def update(mass=p, bm=p, bmin=p, mp=p, N=5, rows=p, td=p, B=4, alpha=0.6, eps=1e-6):
        return lib.m3l_replay_per_update(mass, bm, bmin, mp, N, rows, td, B, alpha, eps, None)

    def add(mass=p, bm=p, bmin=p, mp=p, N=14, first=0, n_set=2, n_zero=0, alpha=0.6):
        return lib.m3l_replay_per_add(mass, bm, bmin, mp, N, first, n_set, n_zero, alpha, None)
    limit = P.PER_MAX_ROWS
    for fn, who, cases in (
            (sample, "replay_per_sample", ((dict(mass=None), "NULL"), (dict(bmin=None), "NULL"), (dict(u=None), "NULL"), (dict(rows=None), "NULL"),
                                           (dict(w=None), "NULL"), (dict(N=0), "N=0"), (dict(N=limit + 1), f"N={limit + 1}"), (dict(B=0), "B=0"),
                                           (dict(beta=-0.5), "beta=-0.5"), (dict(beta=float("nan")), "beta=nan"), (dict(mass=p + 4), "16-byte"))),
            (update, "replay_per_update", ((dict(mp=None), "NULL"), (dict(rows=None), "NULL"), (dict(td=None), "NULL"), (dict(bm=None), "NULL"),
                                           (dict(B=0), "B=0"), (dict(B=P.PER_MAX_UPDATE + 1), f"B={P.PER_MAX_UPDATE + 1}"), (dict(alpha=1.5), "alpha=1.5"),
                                           (dict(eps=0.0), "priority_eps=0"), (dict(eps=float("inf")), "priority_eps=inf"), (dict(N=limit + 1), "N="))),
            (add, "replay_per_add", ((dict(mp=None), "NULL"), (dict(first=14), "first_row=14"), (dict(first=-1), "first_row=-1"), (dict(n_set=0), "n_set=0"),
                                     (dict(n_set=8, n_zero=8), "n_zero=8"), (dict(alpha=-1.0), "alpha=-1"), (dict(mass=None), "NULL")))):
        for kw, msg in cases:
            assert fn(**kw) == 1 and msg in L.last_error() and who in L.last_error(), (who, kw, L.last_error())
    assert lib.m3l_replay_per_refresh(None, 5, p, p, None) == 1 and "replay_per_refresh: NULL" in L.last_error()
    assert lib.m3l_replay_per_refresh(p, limit + 1, p, p, None) == 1 and "replay_per_refresh: N=" in L.last_error()
    for kw, msg in ((dict(B=0), "B=0"), (dict(td_abs=None), "null"), (dict(q=None), "null")):
        a = dict(q=p, t=p, w=None, B=4, loss=p, coef=p, td_abs=p)
        a.update(kw)
        assert lib.m3l_sac_critic_loss_w_fwd(a["q"], a["t"], a["w"], a["B"], a["loss"], a["coef"], a["td_abs"], None) == 1
        assert msg in L.last_error() and "sac_critic_loss_w_fwd" in L.last_error()
