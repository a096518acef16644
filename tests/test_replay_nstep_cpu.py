"""CPU-only checks of n-step returns (DeviceReplayBuffer(n_steps=, gamma=), m3l_replay_nstep_rows, the *_rows2 gathers,
m3l_sac_td_target_rows): the restatement of tests/nstep_cases.py against walks written out by hand, the coverage condition of the stream that
test_replay_nstep_gpu.py runs, the rejections of the constructor and of the entry points before any launch, and the ABI.  No kernel is
launched here."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import m3l_amd
import nstep_cases as NC
import replay_cases as PC
from m3l_amd import _lib as L
from m3l_amd import replay as P

NEW_SYMBOLS = ("m3l_replay_nstep_rows", "m3l_replay_gather_load_rows2", "m3l_replay_gather_load_frames_rows2", "m3l_sac_td_target_rows")
F32 = np.float32


def _header():
    return open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "m3l_amd.h")).read()


def _declared(hdr, name):
    """The parameter list of `int name(...)` in the header, split at its commas."""
    m = re.search(r"\bint " + name + r"\(([^)]*)\)", hdr)
    assert m, name
    return [" ".join(p.split()) for p in m.group(1).split(",")]


def _ctype_of(param):
    if "*" in param:
        return (C.c_void_p, C.POINTER(L.SacDesc))
    return {"int": (C.c_int,), "long": (C.c_long,), "float": (C.c_float,), "double": (C.c_double,)}[param.split()[0]]


def test_exports_and_abi():
    assert L.lib().m3l_version() >= 414
    hdr = _header()
    assert "n-step returns (ABI 414)" in hdr
    for name in NEW_SYMBOLS:
        assert name in L.EXPORTS and hasattr(L.lib(), name)
        res, args = L._SIGS[name]
        params = _declared(hdr, name)
        assert res is C.c_int and len(args) == len(params), (name, len(args), len(params))
        for a, p in zip(args, params):
            assert a in _ctype_of(p), (name, p, a)
    # the new entries are their neighbours with the arguments the issue names, in the header's order
    rows, nstep = _declared(hdr, "m3l_replay_gather_rows"), _declared(hdr, "m3l_replay_nstep_rows")
    assert nstep[:12] == rows[:12] and nstep[12:15] == ["int n_steps", "float gamma", "int newest"]
    assert nstep[15:] == ["float* actions_out", "float* rewards_out", "float* dones_out", "float* discounts_out", "int64_t* rows_out",
                          "int64_t* next_rows_out", "void* stream"]
    for one, two in (("m3l_replay_gather_load", "m3l_replay_gather_load_rows2"), ("m3l_replay_gather_load_frames", "m3l_replay_gather_load_frames_rows2")):
        a, b = _declared(hdr, one), _declared(hdr, two)
        assert b[:-3] == a[:-2] and b[-3:] == ["const int64_t* next_rows", "int B", "void* stream"], two
    td, td_rows = _declared(hdr, "m3l_sac_td_target"), _declared(hdr, "m3l_sac_td_target_rows")
    assert td_rows == [p if p != "float gamma" else "const float* discounts" for p in td]
    assert "NStepReplayBatch" in m3l_amd.__all__
    assert m3l_amd.NStepReplayBatch._fields == m3l_amd.ReplayBatch._fields + ("discounts", "next_rows")
    assert m3l_amd.ReplayBatch._fields == ("observations", "actions", "next_observations", "dones", "rewards", "rows")


# ---- the restatement against walks written out by hand: T = 6 steps, one environment, gamma = 0.5 (every power exact)
def _hand(dones, timeouts, rewards):
    T = len(dones)
    col = lambda v: np.asarray(v, dtype=F32).reshape(T, 1)      # noqa: E731
    return dict(actions=np.arange(T, dtype=F32).reshape(T, 1, 1), rewards=col(rewards), dones=col(dones), timeouts=None if timeouts is None else col(timeouts))


def test_walk_ended_by_a_done_at_the_sampled_step():
    s = _hand([0, 0, 1, 0, 0, 0], [0, 0, 0, 0, 0, 0], [1, 2, 4, 8, 16, 32])
    ref = NC.nstep_reference(s, [2], [0], 6, 3, 0.5, newest=5)
    assert ref["k_star"].tolist() == [0] and ref["last"].tolist() == [2] and ref["kind"] == ["done"]
    assert ref["rewards"].tolist() == [[4.0]] and ref["dones"].tolist() == [[1.0]] and ref["discounts"].tolist() == [[0.5]]
    assert ref["rows"].tolist() == [2] and ref["next_rows"].tolist() == [2] and ref["actions"].tolist() == [[2.0]]
    # the same step truncated: done is masked to 0 and the walk still ends there
    s = _hand([0, 0, 1, 0, 0, 0], [0, 0, 1, 0, 0, 0], [1, 2, 4, 8, 16, 32])
    ref = NC.nstep_reference(s, [2, 1], [0, 0], 6, 3, 0.5, newest=5)
    assert ref["kind"] == ["truncated", "truncated"] and ref["k_star"].tolist() == [0, 1] and ref["dones"].tolist() == [[0.0], [0.0]]
    assert ref["rewards"].tolist() == [[4.0], [2 + 0.5 * 4]] and ref["discounts"].tolist() == [[0.5], [0.25]]
    # without timeout handling the done stays
    s["timeouts"] = None
    assert NC.nstep_reference(s, [1], [0], 6, 3, 0.5, newest=5)["dones"].tolist() == [[1.0]]


def test_walk_ended_by_the_write_head():
    """A full ring with pos = 2: step 1 was written last, steps 2.. hold the oldest data.  The walk from step 5 wraps the ring end and stops at 1."""
    s = _hand([0, 0, 0, 0, 0, 0], [0, 0, 0, 0, 0, 0], [1, 2, 4, 8, 16, 32])
    ref = NC.nstep_reference(s, [5, 1, 0], [0, 0, 0], 6, 5, 0.5, newest=1)
    assert ref["kind"] == ["write_head"] * 3 and ref["k_star"].tolist() == [2, 0, 1] and ref["last"].tolist() == [1, 1, 1]
    assert ref["wrapped"].tolist() == [True, False, False]
    assert ref["rewards"].tolist() == [[32 + 0.5 * 1 + 0.25 * 2], [2.0], [1 + 0.5 * 2]]
    assert ref["discounts"].tolist() == [[0.125], [0.5], [0.25]] and ref["dones"].tolist() == [[0.0]] * 3      # it bootstraps from next_obs[1]
    assert ref["next_rows"].tolist() == [1, 1, 1] and ref["rows"].tolist() == [5, 1, 0]


def test_full_walk_and_the_reward_normalisation():
    s = _hand([0, 0, 0, 1, 0, 0], [0, 0, 0, 0, 0, 0], [1, -2, 4, 8, 16, 32])
    ref = NC.nstep_reference(s, [0, 1], [0, 0], 6, 3, 0.5, newest=5)
    assert ref["kind"] == ["full", "done"] and ref["k_star"].tolist() == [2, 2] and ref["last"].tolist() == [2, 3]
    assert ref["rewards"].tolist() == [[1 - 1 + 1], [-2 + 2 + 2]] and ref["discounts"].tolist() == [[0.125], [0.125]]
    assert ref["dones"].tolist() == [[0.0], [1.0]]
    # var + eps = 4 -> scale 2, clip 1.5: r~ = 0.5, -1, 1.5 (clipped from 2), 1.5 (from 4)
    ref = NC.nstep_reference(s, [0, 1], [0, 0], 6, 3, 0.5, newest=5, reward_norm=(4.0, 0.0, 1.5))
    assert ref["rewards"].tolist() == [[0.5 - 0.5 + 0.375], [-1 + 0.75 + 0.375]]
    assert ref["reward_bound"].tolist() == [[6 * 2.0 ** -23 * (0.5 + 0.5 + 0.375)], [6 * 2.0 ** -23 * (1 + 0.75 + 0.375)]]
    # n_steps = 1 is the one-step sample
    one = NC.nstep_reference(s, [0, 3], [0, 0], 6, 1, 0.99, newest=5)
    assert one["k_star"].tolist() == [0, 0] and one["rewards"].tolist() == [[1.0], [8.0]] and one["next_rows"].tolist() == [0, 3]
    assert one["discounts"].tolist() == [[float(F32(0.99))]] * 2


def test_next_observations_are_those_of_the_last_step():
    T, E = 5, 2
    rng = np.random.default_rng(3)
    stores = {"image": rng.integers(0, 256, (T, E, 2, 4, 4, 3), dtype=np.uint8)}
    nstores = {"image": rng.integers(0, 256, (T, E, 2, 4, 4, 3), dtype=np.uint8)}
    s = PC.make_replay_scalars(T, E, 2, seed=4)
    s["dones"][:] = 0
    s["dones"][3, 1] = 1
    t, e = np.array([4, 2, 0]), np.array([0, 1, 1])
    ref = NC.sample_reference(stores, nstores, s, t, e, T, 3, 0.9, newest=1)
    assert ref["last"].tolist() == [1, 3, 1] and ref["kind"] == ["write_head", "done", "write_head"]
    obs = PC.sample_reference(stores, nstores, s, t, e, T)["observations"]["image"]
    nxt = PC.sample_reference(stores, nstores, s, ref["last"], e, T)["next_observations"]["image"]
    np.testing.assert_array_equal(ref["observations"]["image"], obs)
    np.testing.assert_array_equal(ref["next_observations"]["image"], nxt)


# ---- the coverage condition of the GPU test's stream
@pytest.mark.parametrize("n", NC.N_STEPS)
def test_the_gpu_stream_meets_every_kind_of_walk_end(n):
    """Over the valid (t, e) of the three checkpoints, for every n_steps tested: every kind of walk end occurs, and for n > 1 at least one walk
    wraps the ring end.  The episodes do not depend on the frame stack or the shapes.  The frame-deduplicated buffer samples fewer steps of a
    full ring (not its fs - 1 oldest): it still meets every kind, except that a ring of 7 with a frame stack of 4 has no room for a full walk
    of 5 (4 valid steps when full, newest = 4 at the first checkpoint)."""
    U8 = np.uint8
    for fs in (1, 2, 4):
        st = NC.make_stream(fs, (2, 2), None, 0, U8, None, seed=fs)
        kinds, wraps = NC.coverage(st, n)
        assert kinds == set(NC.KINDS) and (wraps >= 1 or n == 1), (n, fs, kinds, wraps)
        kinds, wraps = NC.coverage(st, n, timeouts=False)
        assert kinds == {"done", "write_head", "full"}, (n, fs, kinds)
        kinds, wraps = NC.coverage(st, n, fs=fs)
        want = set(NC.KINDS) - ({"full"} if (n, fs) == (5, 4) else set())
        assert kinds == want and (wraps >= 1 or n == 1), (n, fs, kinds, wraps)


# ---- rejections
SHAPES = {"image": (2, 8, 8, 3), "tactile": (2, 6, 4, 4)}
DTYPES = {"image": np.uint8, "tactile": np.float32}


def _buffer(**kw):
    args = dict(buffer_size=14, n_envs=2, obs_shapes=SHAPES, obs_dtypes=DTYPES, action_dim=3)
    args.update(kw)
    return m3l_amd.DeviceReplayBuffer(**args)


def test_constructor():
    buf = _buffer()
    assert (buf.n_steps, buf.gamma) == (1, 0.99)
    buf = _buffer(n_steps=7, gamma=1.0, frame_dedup=True)
    assert (buf.n_steps, buf.gamma, buf.buffer_size) == (7, 1.0, 7)
    assert _buffer(n_steps=np.int64(3), gamma=np.float32(0.5)).gamma == 0.5
    for bad in (0, -1, 8, 2.0, "3", None, True):
        with pytest.raises(ValueError, match=r"n_steps=.* must be an integer from 1 to the capacity in steps \(7\)"):
            _buffer(n_steps=bad)
    for bad in (0.0, -0.5, 1.0001, float("nan"), float("inf"), "0.9", None):
        with pytest.raises(ValueError, match=r"gamma=.* must be a number in \(0, 1\]"):
            _buffer(n_steps=2, gamma=bad)
    with pytest.raises(ValueError, match="n_steps > 1 needs optimize_memory_usage=False"):
        _buffer(n_steps=2, optimize_memory_usage=True, handle_timeout_termination=False)
    # the single-store buffer itself is as before
    assert _buffer(n_steps=1, optimize_memory_usage=True, handle_timeout_termination=False).n_steps == 1


def test_functional_forms_refuse_host_tensors_and_bad_arguments():
    rows = torch.zeros(2, dtype=torch.int64)
    with pytest.raises(m3l_amd.M3LError, match="must live on the GPU"):
        P.nstep_rows(torch.zeros(3, 2, 1), torch.zeros(3, 2), torch.zeros(3, 2), None, rows, 2, 0.99, 0)
    with pytest.raises(m3l_amd.M3LError, match="must live on the GPU"):
        P.gather_load(torch.zeros(3, 2, 1, 4, 4, 3), None, rows, next_rows=rows)
    with pytest.raises(m3l_amd.M3LError, match="must live on the GPU"):
        P.gather_load_frames(torch.zeros(3, 2, 4, 4, 3), None, torch.zeros(3, 2, dtype=torch.int32), rows, next_rows=rows, frame_stack=2)


def test_nstep_rows_entry_point_refuses_bad_arguments():
    lib = L.lib()
    p = 1 << 20

    def rc(actions=p, rewards=p, dones=p, timeouts=p, T=3, n_envs=2, A=2, rows=p, shift=0, B=4, scale=0.0, clip=0.0, n=2, gamma=0.99, newest=0, out=p,
           disc=p, rows_out=p, next_rows_out=p):
        return lib.m3l_replay_nstep_rows(actions, rewards, dones, timeouts, T, n_envs, A, rows, shift, B, scale, clip, n, gamma, newest, out, out, out,
                                         disc, rows_out, next_rows_out, None)
    for kw, msg in ((dict(A=0), "A=0"), (dict(B=0), "B=0"), (dict(T=0), "T=0"), (dict(rewards=None), "NULL"), (dict(dones=None), "NULL"),
                    (dict(out=None), "NULL"), (dict(rows=None), "NULL"), (dict(disc=None), "NULL"), (dict(rows_out=None), "NULL"),
                    (dict(next_rows_out=None), "NULL"), (dict(shift=6), "row_shift=6"), (dict(scale=-1.0), "reward_scale=-1"),
                    (dict(scale=2.0, clip=-1.0), "reward_clip=-1"), (dict(n=0), "n_steps=0"), (dict(n=4), "n_steps=4"), (dict(gamma=0.0), "gamma=0"),
                    (dict(gamma=1.5), "gamma=1.5"), (dict(gamma=float("nan")), "gamma=nan"), (dict(newest=3), "newest=3"), (dict(newest=-1), "newest=-1")):
        assert rc(**kw) == 1 and msg in L.last_error() and "replay_nstep_rows" in L.last_error(), (kw, L.last_error())


def test_rows2_entry_points_refuse_a_missing_row_list():
    lib = L.lib()
    p = 1 << 20
    outs = (C.c_void_p * 16)(*([1 << 24] * 16))
    head = (p, p, 0, 8, 8, 0.0, 1.0, p, p, p, p, 0, 4, 4, 2, -1.0, 1.0, outs, outs)
    assert lib.m3l_replay_gather_load_rows2(*head, 3, 2, 2, p, 0, None, 4, None) == 1
    assert "replay_gather_load_rows2: next_rows is NULL" in L.last_error()
    assert lib.m3l_replay_gather_load_rows2(*head, 3, 2, 2, p, 6, p, 4, None) == 1
    assert "replay_gather_load_rows2: row_shift=6" in L.last_error()
    assert lib.m3l_replay_gather_load_frames_rows2(*head, p, 3, 2, 2, p, 0, None, 4, None) == 1
    assert "replay_gather_load_frames_rows2: next_rows is NULL" in L.last_error()
    assert lib.m3l_replay_gather_load_frames_rows2(*head, None, 3, 2, 2, p, 0, p, 4, None) == 1
    assert "replay_gather_load_frames_rows2: ages is NULL" in L.last_error()
    assert lib.m3l_sac_td_target_rows(None, 4, p, p, p, p, None, 0.1, None, p, None) == 1
    assert "sac_td_target_rows: discounts is NULL" in L.last_error()
