"""n-step returns of the device-resident replay buffer on a real MI355X (m3l_amd/replay.py `n_steps=`, csrc/replay.hip m3l_replay_nstep_rows,
m3l_replay_gather_load_rows2, m3l_replay_gather_load_frames_rows2).

One stream of add() calls (tests/nstep_cases.py: T = 7 steps of 2 environments, whose episodes meet every kind of walk end for every n_steps —
test_replay_nstep_cpu.py checks that) goes into a default buffer, into stacked buffers with n_steps 1, 2, 3 and 5 and into frame-deduplicated
ones, and after 5, 7 and 17 adds `sample(indices=...)` runs over every valid (t, e):
  1. n_steps = 1: the bits of the default buffer in every field; nstep_rows called with n_steps = 1 gives gather_rows' bits and discounts = g
  2. stacked against the float64 restatement: observations, next_observations, actions, dones, rows, next_rows exact; rewards within
     2 n 2^-23 sum_k |g^k r~_k| per sample and discounts within n 2^-23 relative — n float32 products and n - 1 float32 sums, each within
     2^-24 relative, with a factor 2 of margin; a walk of no move gives the float32 reward and g themselves
  3. frame-deduplicated against stacked: equal bits in every field
  4. -1 / out-of-range entries of rows or next_rows at the functional level: that half is NaN, the other half and the neighbours intact
  5. two runs, equal bits
Shapes are the smallest that reach every path: pixel counts that are (8 x 8, 3 x 4 x 4) and are not (5 x 5, 3 x 5 x 3) a multiple of the
4-element vector, uint8 and float32 stores, one and three sensors, frame stacks 1, 2 and 4, with and without timeout handling and reward
normalisation."""
import numpy as np
import pytest
import torch

import memguard as MG
import nstep_cases as NC
import replay_frame_cases as FC

pytestmark = pytest.mark.gpu

import m3l_amd  # noqa: E402
from m3l_amd import replay as P  # noqa: E402

DEV = "cuda:0"
T, E, A = NC.T, NC.E, NC.A
U8, F32 = np.uint8, np.float32
GAMMA = 0.97
G32 = float(np.float32(GAMMA))
RANGES = ((0.1, 0.9), (-2, 3))          # ranges floats cannot represent

# name -> image (H, W), tactile (h, w), sensors, (image, tactile) dtypes, timeout handling, reward normalisation
CONFIGS = {
    "u8_8x8_f32_4x4_S1_timeouts_raw": ((8, 8), (4, 4), 1, (U8, F32), True, False),
    "f32_5x5_u8_5x3_S3_plain_norm": ((5, 5), (5, 3), 3, (F32, U8), False, True),
    "f32_8x8_f32_4x4_S3_timeouts_norm": ((8, 8), (4, 4), 3, (F32, F32), True, True),
    "u8_5x5_u8_5x3_S1_plain_raw": ((5, 5), (5, 3), 1, (U8, U8), False, False),
}


def _buffer(cfg, fs, **kw):
    image_hw, tactile_hw, S, dtypes, timeouts, _ = cfg
    shapes = {"image": (fs,) + image_hw + (3,), "tactile": (fs, 3 * S) + tactile_hw}
    dts = {"image": dtypes[0], "tactile": dtypes[1]}
    return m3l_amd.DeviceReplayBuffer(T * E, E, shapes, dts, A, handle_timeout_termination=timeouts, image_normalization=list(RANGES[0]),
                                      tactile_normalization=list(RANGES[1]), device=DEV, **kw)


def _add(buf, st, k):
    buf.add({key: v[k] for key, v in st["obs"].items()}, {key: v[k] for key, v in st["next_obs"].items()}, st["actions"][k], st["rewards"][k],
            st["dones"][k], st["infos"][k])


def _same_obs(got, want, what):
    assert isinstance(got, m3l_amd.LoadedObs) and sorted(got) == sorted(want), what
    for k in want:
        w = torch.from_numpy(np.ascontiguousarray(want[k])).to(DEV)
        assert got[k].dtype == torch.float32 and got[k].shape == w.shape, (what, k)
        assert torch.equal(got[k], w), f"{what}: {k} differs in {(got[k] != w).sum().item()} of {w.numel()} elements"


def _exact(got, want, what):
    want = torch.from_numpy(np.ascontiguousarray(want))
    assert got.shape == want.shape and got.dtype == want.dtype and torch.equal(got.cpu(), want), what


def _check_against_restatement(batch, ref, n, what):
    """Check 2 -> (largest reward error over its bound, largest relative discount error over its bound)."""
    assert isinstance(batch, m3l_amd.NStepReplayBatch)
    _same_obs(batch.observations, ref["observations"], what + " observations")
    _same_obs(batch.next_observations, ref["next_observations"], what + " next_observations")
    for name in ("actions", "dones", "rows", "next_rows"):
        _exact(getattr(batch, name), ref[name], f"{what} {name}")
    B = len(ref["rows"])
    assert batch.rewards.shape == batch.discounts.shape == (B, 1) and batch.rewards.dtype == batch.discounts.dtype == torch.float32
    r, d = batch.rewards.double().cpu().numpy(), batch.discounts.double().cpu().numpy()
    r_err, d_err = np.abs(r - ref["rewards"]), np.abs(d - ref["discounts"]) / ref["discounts"]
    r_ratio = float((r_err / np.maximum(ref["reward_bound"], 1e-300)).max())
    d_ratio = float(d_err.max() / (n * NC.EPS))
    print(f"[{what}] rewards: largest error / bound {r_ratio:.3f}; discounts: largest relative error {d_err.max():.2e} (bound {n * NC.EPS:.2e})")
    assert (r_err <= ref["reward_bound"]).all(), (what, r_ratio)
    assert (d_err <= n * NC.EPS).all(), (what, d_ratio)
    still = ref["k_star"] == 0                      # a walk of no move: the one-step reward and gamma, bit for bit
    assert np.array_equal(r[still], ref["rewards"][still]) and (d[still] == G32).all(), what
    return r_ratio, d_ratio


@pytest.mark.parametrize("fs", [1, 2, 4])
@pytest.mark.parametrize("name", sorted(CONFIGS))
def test_nstep_buffers_over_every_valid_step(name, fs):
    """Checks 1, 2, 3 and 5 of the module docstring at the three checkpoints.  Measured on an MI355X (EXPERIMENTS.md 5.24): see there."""
    cfg = CONFIGS[name]
    image_hw, tactile_hw, S, dtypes, timeouts, norm = cfg
    st = NC.make_stream(fs, image_hw, tactile_hw, S, dtypes[0], dtypes[1], seed=sorted(CONFIGS).index(name) * 10 + fs)
    env = NC.RewardNorm() if norm else None
    default = _buffer(cfg, fs)
    stacked = {n: _buffer(cfg, fs, n_steps=n, gamma=GAMMA) for n in NC.N_STEPS}
    dedup = {n: _buffer(cfg, fs, n_steps=n, gamma=GAMMA, frame_dedup=True) for n in NC.N_STEPS}
    kinds = {n: set() for n in NC.N_STEPS}
    for k in range(max(NC.CHECKPOINTS)):
        for buf in [default] + list(stacked.values()) + list(dedup.values()):
            _add(buf, st, k)
        if k + 1 not in NC.CHECKPOINTS:
            continue
        what = f"{name} fs={fs} after {k + 1} adds"
        smodel, fmodel = FC.fill_models(k + 1, T, fs, False, st)
        stores, nstores, scalars = FC.stacked_stores(smodel, st)
        if not timeouts:
            scalars["timeouts"] = None
        newest = (smodel.pos - 1) % T
        t, e = NC.valid_pairs(smodel)
        td, ed = NC.valid_pairs(fmodel)
        # 1. n_steps = 1 is the default buffer, and nstep_rows with n_steps = 1 is gather_rows
        base, one = default.sample(1, env=env, indices=(t, e)), stacked[1].sample(1, env=env, indices=(t, e))
        assert type(one) is m3l_amd.ReplayBatch and not MG.differing(list(base), list(one)), what
        rows = torch.from_numpy(t * E + e).to(DEV)
        scale, clip = P.reward_normalization(env)
        b = default
        by_walk = P.nstep_rows(b.actions, b.rewards, b.dones, b.timeouts, rows, 1, GAMMA, newest, scale, clip)
        by_rows = P.gather_rows(b.actions, b.rewards, b.dones, b.timeouts, rows, scale, clip, return_rows=True)
        assert not MG.differing(list(by_rows), [by_walk[0], by_walk[1], by_walk[2], by_walk[4]]), what
        assert torch.equal(by_walk[5], rows) and (by_walk[3] == G32).all() and by_walk[3].shape == (len(t), 1), what
        assert torch.equal(by_walk[1], base.rewards) and torch.equal(by_walk[2], base.dones)
        for n in NC.N_STEPS[1:]:
            # 2. the stacked buffer against the restatement
            ref = NC.sample_reference(stores, nstores, scalars, t, e, T, n, GAMMA, newest, env.triple() if norm else None, *RANGES)
            kinds[n] |= set(ref["kind"])
            batch = stacked[n].sample(1, env=env, indices=(t, e))
            _check_against_restatement(batch, ref, n, f"{what} n_steps={n}")
            # 5. two runs
            assert not MG.differing(list(batch), list(stacked[n].sample(1, env=env, indices=(t.copy(), torch.from_numpy(e))))), what
            # 3. the frame-deduplicated buffer against the stacked one, over its own valid steps
            got, want = dedup[n].sample(1, env=env, indices=(td, ed)), stacked[n].sample(1, env=env, indices=(td, ed))
            assert isinstance(got, m3l_amd.NStepReplayBatch) and got._fields == want._fields
            bad = MG.differing(list(got), list(want))
            assert not bad, f"{what} n_steps={n}: frame_dedup differs from the stacked buffer in fields {bad}"
            assert not MG.differing(list(got), list(dedup[n].sample(1, env=env, indices=(td, ed)))), what
            assert not MG.nonfinite(list(got)) and not MG.nonfinite(list(batch))
        got, want = dedup[1].sample(1, env=env, indices=(td, ed)), stacked[1].sample(1, env=env, indices=(td, ed))
        assert type(got) is m3l_amd.ReplayBatch and not MG.differing(list(got), list(want)), what
    for n in NC.N_STEPS[1:]:
        assert kinds[n] == set(NC.KINDS) - (set() if timeouts else {"truncated"}), (n, kinds[n])


def _filled(cfg, fs, n, n_adds=17, seed=7, **kw):
    image_hw, tactile_hw, S, dtypes, _, _ = cfg
    st = NC.make_stream(fs, image_hw, tactile_hw, S, dtypes[0], dtypes[1], seed=seed)
    bufs = _buffer(cfg, fs, n_steps=n, gamma=GAMMA, **kw), _buffer(cfg, fs, n_steps=n, gamma=GAMMA, frame_dedup=True, **kw)
    for k in range(n_adds):
        for buf in bufs:
            _add(buf, st, k)
    return st, bufs


@pytest.mark.parametrize("name", ["u8_8x8_f32_4x4_S1_timeouts_raw", "f32_5x5_u8_5x3_S3_plain_norm"])
def test_wrong_entries_of_either_row_list_give_nan_halves(name):
    """Check 4.  fs = 4, n_steps = 3, a full ring with pos = 3: rows and next_rows as nstep_rows writes them, then -1, T n_envs and +-2^40 put into
    one list at a time.  A wrong entry of rows blanks the observation of that sample alone, a wrong entry of next_rows its next observation
    alone; nstep_rows itself answers a wrong row with NaN and -1 and leaves its neighbours intact."""
    fs, n = 4, 3
    _, (sbuf, dbuf) = _filled(CONFIGS[name], fs, n)
    first, count = dbuf._valid_steps()
    valid = [(first + u) % T for u in range(count)]
    rows = torch.tensor([s * E + x for s in valid for x in range(E)], dtype=torch.int64, device=DEV)
    B = rows.numel()
    assert B == 8 and sbuf.pos == 3
    newest = 2
    clean = P.nstep_rows(sbuf.actions, sbuf.rewards, sbuf.dones, sbuf.timeouts, rows, n, GAMMA, newest)
    next_rows = clean[5]
    assert torch.equal(clean[4], rows) and not torch.equal(next_rows, rows)
    bad_rows, bad_next = rows.clone(), next_rows.clone()
    bad_rows[1], bad_rows[3], bad_rows[6] = -1, T * E, 2 ** 40
    bad_next[2], bad_next[4], bad_next[6] = T * E, -1, -2 ** 40
    in_rows = torch.tensor([i in (1, 3, 6) for i in range(B)], device=DEV)
    in_next = torch.tensor([i in (2, 4, 6) for i in range(B)], device=DEV)

    def gathers(r, nr):
        so, sn = sbuf.observations, sbuf.next_observations
        do, dn = dbuf.frames, dbuf.next_frames
        return (P.gather_load(so["image"], so["tactile"], r, sn["image"], sn["tactile"], *RANGES, next_rows=nr),
                P.gather_load_frames(do["image"], do["tactile"], dbuf.ages, r, dn["image"], dn["tactile"], *RANGES, next_rows=nr, frame_stack=fs))
    want = gathers(rows, next_rows)
    assert not MG.differing([dict(x) for x in want[0]], [dict(x) for x in want[1]]) and not MG.nonfinite([dict(x) for x in want[0]])
    for (obs, nob), (wobs, wnob), form in zip(gathers(bad_rows, bad_next), want, ("stacked", "frames")):
        for key in wobs:
            assert torch.isnan(obs[key][in_rows]).all() and torch.equal(obs[key][~in_rows], wobs[key][~in_rows]), (form, key, "observations")
            assert torch.isnan(nob[key][in_next]).all() and torch.equal(nob[key][~in_next], wnob[key][~in_next]), (form, key, "next_observations")
    got = P.nstep_rows(sbuf.actions, sbuf.rewards, sbuf.dones, sbuf.timeouts, bad_rows, n, GAMMA, newest)
    for g, w in zip(got[:4], clean[:4]):
        assert torch.isnan(g[in_rows]).all() and torch.equal(g[~in_rows], w[~in_rows])
    for g, w in zip(got[4:], clean[4:]):
        assert (g[in_rows] == -1).all() and torch.equal(g[~in_rows], w[~in_rows])
    # every row_shift agrees with rows shifted on the host; next_rows takes no shift
    every = torch.arange(T * E, dtype=torch.int64, device=DEV)
    for shift in (1, 5, T * E - 1):
        shifted = P.nstep_rows(sbuf.actions, sbuf.rewards, sbuf.dones, sbuf.timeouts, every, n, GAMMA, newest, row_shift=shift)
        on_host = P.nstep_rows(sbuf.actions, sbuf.rewards, sbuf.dones, sbuf.timeouts, (every + shift) % (T * E), n, GAMMA, newest)
        assert not MG.differing(list(shifted), list(on_host)), shift


def test_drawn_batches_and_rejections():
    """A drawn batch (no indices) of the full frame-deduplicated ring — its draw is relative to the first valid step, so the kernels apply a
    row shift — is the batch its own rows name, its rows cover the valid set and nothing else; and what the buffer refuses."""
    fs, n = 2, 3
    cfg = CONFIGS["u8_8x8_f32_4x4_S1_timeouts_raw"]
    _, (sbuf, dbuf) = _filled(cfg, fs, n)
    first, count = dbuf._valid_steps()
    assert (first, count) == (4, 6)
    torch.manual_seed(5)
    batch = dbuf.sample(512)
    rows = batch.rows.cpu().numpy()
    assert set(rows.tolist()) == {((first + u) % T) * E + x for u in range(count) for x in range(E)}
    assert batch.next_rows.dtype == torch.int64 and batch.discounts.shape == (512, 1)
    again = sbuf.sample(1, indices=(rows // E, rows % E))
    assert not MG.differing(list(batch), list(again))
    drawn = sbuf.sample(64)                                # the stacked ring draws over all T steps
    assert isinstance(drawn, m3l_amd.NStepReplayBatch) and int(drawn.rows.min()) >= 0 and int(drawn.rows.max()) < T * E
    assert not MG.nonfinite(list(drawn)) and not MG.differing(list(drawn), list(sbuf.sample(1, indices=(drawn.rows.cpu() // E, drawn.rows.cpu() % E))))
    with pytest.raises(ValueError, match="n_steps > 1 needs optimize_memory_usage=False"):
        _buffer((cfg[0], cfg[1], cfg[2], cfg[3], False, False), fs, n_steps=2, optimize_memory_usage=True)
    with pytest.raises(ValueError, match="indices name steps outside"):
        dbuf.sample(1, indices=([3], [0]))
    with pytest.raises(ValueError, match="next_rows must be a contiguous int64 tensor of rows' shape"):
        P.gather_load(sbuf.observations["image"], None, batch.rows, sbuf.next_observations["image"], next_rows=batch.next_rows[:-1])
    with pytest.raises(ValueError, match="next_rows must be a contiguous int64 tensor of rows' shape"):
        P.gather_load_frames(dbuf.frames["image"], None, dbuf.ages, batch.rows, next_rows=batch.next_rows.to(torch.int32), frame_stack=fs)
    with pytest.raises(ValueError, match=r"n_steps=8 must be an integer in \[1, 7\]"):
        P.nstep_rows(sbuf.actions, sbuf.rewards, sbuf.dones, sbuf.timeouts, batch.rows, 8, GAMMA, 0)
    with pytest.raises(ValueError, match=r"gamma=0.0 must lie in \(0, 1\]"):
        P.nstep_rows(sbuf.actions, sbuf.rewards, sbuf.dones, sbuf.timeouts, batch.rows, 2, 0.0, 0)
    with pytest.raises(ValueError, match="newest=7 must be a step of the ring"):
        P.nstep_rows(sbuf.actions, sbuf.rewards, sbuf.dones, sbuf.timeouts, batch.rows, 2, GAMMA, 7)
