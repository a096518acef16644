"""Prioritised replay on a real MI355X (m3l_amd/replay.py `prioritized=`, csrc/replay.hip m3l_replay_per_refresh / _add / _sample / _update,
csrc/sac.hip m3l_sac_critic_loss_w_fwd) against the float64 restatement of tests/per_cases.py (parity unpinned).

  1. exact arithmetic: integer leaves in [0, 8], B a power of two that divides the total, u multiples of 2^-8 — every float32 operation of the
     path is exact (test_replay_per_cpu.py asserts it, and that targets fall on leaf and block boundaries), so `rows` equals the restatement's
     for every sample, stratified or not, and the block sums and minima equal it too; N = 3 PER_BLOCK + 5 and N = 5, and one case of
     257 PER_BLOCK + 3 rows, at which a thread of the sampler sums a chunk of two blocks into the block prefix
  2. general masses (a ratio of 10^6, a fifth zero): every row has positive mass and the float64 target lies in [C[r - 1] - tol, C[r] + tol];
     weights and updated masses within REL of float64
  3. per_update: duplicates, NaN / inf, rows outside the structure, rows of zero mass, max_priority, the touched blocks bit-equal to a full
     refresh, the untouched ones unchanged
  4. the buffer on the stream of tests/nstep_cases.py (T = 7, E = 2) after 5, 7 and 17 adds, stacked / frame_dedup / single-store, n_steps 1, 3
  5. the weighted critic loss against float64 at the SAC head tests' bounds, B = 5 and 300; ones and None give the unweighted bits
  6. two runs of everything give equal bits; the memory contract (tests/memguard.py) of every new entry

tol.  With eps = 2^-24 and every partial sum at most `total`, the float32 operations between the leaves and the comparison `p[r] > residual`:
  block sums      2 (four leaves of a thread) + 6 (butterfly of the wave) + 2 (four waves)                                     10
  block prefix    1 (running sum of a thread's chunk of one block at these sizes) + 6 (wave scan) + 3 (waves in front) + 1 + 1  12
  x_k             the total above (22), then k + u, total / B, their product                                                    25
  residual        the prefix in front of the block (22) and one subtraction                                                     23
  leaf prefix     16 (running sum of a lane's leaves) + 6 (wave scan) + 1                                                       23
71 operations: tol = 2 * 71 * 2^-24 * total, the factor 2 the margin of the n-step test's convention.
REL.  The HIP math documentation was not at hand where this was written, so powf counts as 4 ulp (an ulp is at most 2^-23 relative); the quotient in front
of it (weights) or the sum |td| + eps (masses) and the conversion are two roundings of 2^-24, passed on by an exponent of at most 1:
REL = 4 * 2^-23 + 2 * 2^-24 = 5 * 2^-23."""
import numpy as np
import pytest
import torch

import memguard as MG
import nstep_cases as NC
import per_cases as PC
import replay_frame_cases as FC

pytestmark = pytest.mark.gpu

import m3l_amd  # noqa: E402
from m3l_amd import replay as P  # noqa: E402
from m3l_amd import sac as S  # noqa: E402

DEV = "cuda:0"
F32 = np.float32
T, E, A = NC.T, NC.E, NC.A
BLK = PC.PER_BLOCK
OPS = 71
REL = 5 * 2.0 ** -23
SAC_TOL = 1e-4                     # VALUE_TOL = GRAD_TOL of test_sac_head_gpu.py


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _structure(mass):
    m = _dev(mass)
    bm, bmin = P.per_refresh(m)
    return m, bm, bmin


def _follows(what, mass, u, rows, weights, beta, stratified=True):
    """Check 2 for one draw: mass (N) float32 as the structure holds it -> the number of rows that differ from the float64 choice."""
    ref = PC.sample_reference(mass, u, beta, stratified)
    rows, weights = rows.cpu().numpy(), weights.double().cpu().numpy()
    m64 = np.asarray(mass, dtype=np.float64).ravel()
    assert rows.shape == (u.size,) and weights.shape == (u.size, 1) and rows.min() >= 0 and rows.max() < m64.size, what
    assert (m64[rows] > 0).all(), f"{what}: rows of zero mass returned: {rows[m64[rows] == 0]}"
    C, tol = ref["C"], 2 * OPS * 2.0 ** -24 * ref["total"]
    lo = np.where(rows > 0, C[np.maximum(rows - 1, 0)], 0.0)
    worst = max(float(np.maximum(lo - ref["x"], ref["x"] - C[rows]).max() / tol), 0.0)      # 0: every target inside its row's interval
    want = PC.weights_reference(mass, rows, beta)
    w_err = float((np.abs(weights - want) / want).max() / REL)
    differ = int((rows != ref["rows"]).sum())
    print(f"[{what}] {differ} of {u.size} rows differ from the float64 choice; target outside its row by at most {worst:.3f} tol; "
          f"weights: largest relative error {w_err:.3f} of the bound {REL:.2e}")
    assert worst <= 1.0, (what, worst)
    assert w_err <= 1.0, (what, w_err)
    return differ, worst, w_err


# ---- 1. exact arithmetic
@pytest.mark.parametrize("name", sorted(PC.exact_cases()))
def test_exact_arithmetic(name):
    mass, u = PC.exact_cases()[name]
    m, bm, bmin = _structure(mass)
    want_bm, want_min = PC.refresh_reference(mass)
    assert np.array_equal(bm.double().cpu().numpy(), want_bm) and np.array_equal(bmin.double().cpu().numpy(), want_min), name
    for stratified in (True, False):
        ref = PC.sample_reference(mass, u, 0.5, stratified)
        rows, weights = P.per_sample(m, bm, bmin, _dev(u), 0.5, stratified)
        got = rows.cpu().numpy()
        bad = np.flatnonzero(got != ref["rows"])
        assert bad.size == 0, f"{name} stratified={stratified}: samples {bad[:8]} give rows {got[bad[:8]]}, the restatement {ref['rows'][bad[:8]]}"
        assert rows.dtype == torch.int64 and weights.shape == (u.size, 1) and weights.dtype == torch.float32
        err = np.abs(weights.double().cpu().numpy() - ref["weights"]) / ref["weights"]
        assert err.max() <= REL, (name, err.max())
        again = P.per_sample(m, bm, bmin, _dev(u), 0.5, stratified)
        assert not MG.differing([rows, weights], list(again)), name
    # beta = 0: weights of one; the given-rows form: the same weights for the same rows
    rows, weights = P.per_sample(m, bm, bmin, _dev(u), 0.0)
    assert (weights == 1).all()
    rows, weights = P.per_sample(m, bm, bmin, _dev(u), 0.5)
    given, w2 = P.per_sample(m, bm, bmin, None, 0.5, rows=rows)
    assert torch.equal(given, rows) and torch.equal(w2, weights)


# ---- 2. general masses
@pytest.mark.parametrize("n,B", [(PC.N_BIG, 512), (PC.N_BIG, 7), (PC.N_SMALL, 16)])
def test_general_masses(n, B):
    """Measured on an MI355X (EXPERIMENTS.md 5.25): the target leaves its row's interval by at most 0.003 tol; 1 of 512 and 1 of 7 stratified rows
    differ from the float64 choice; weights within 0.33 of REL."""
    mass = PC.general_mass(n, seed=n + B)
    m, bm, bmin = _structure(mass)
    bm64, bmin64 = PC.refresh_reference(mass)
    assert np.array_equal(bmin.double().cpu().numpy(), bmin64)
    assert (np.abs(bm.double().cpu().numpy() - bm64) <= 10 * 2.0 ** -24 * bm64).all()
    g = np.random.default_rng(B)
    for stratified in (True, False):
        u = g.random(B).astype(F32)
        u[0], u[-1] = 0.0, F32(1 - 2.0 ** -24)
        rows, weights = P.per_sample(m, bm, bmin, _dev(u), 0.4, stratified)
        _follows(f"general n={n} B={B} stratified={stratified}", mass, u, rows, weights, 0.4, stratified)
        assert not MG.differing([rows, weights], list(P.per_sample(m, bm, bmin, _dev(u), 0.4, stratified)))


# ---- 3. per_update
def test_per_update():
    n, alpha, eps = PC.N_BIG, 0.6, F32(1e-3)
    mass = PC.general_mass(n, seed=3)
    zero_rows, pos_rows = np.flatnonzero(mass == 0), np.flatnonzero(mass > 0)
    g = np.random.default_rng(4)
    # blocks 0, 2 and 3 are touched, block 1 is not; 300 entries: duplicates meet across the tiles of 256 the kernel compares in
    pool = pos_rows[(pos_rows < BLK) | (pos_rows >= 2 * BLK)]
    rows = g.choice(pool[3:], 300, replace=True).astype(np.int64)          # with duplicates of its own; pool[:3] are named below only
    td = (g.standard_normal(300) * 3).astype(F32)
    rows[0], rows[5], rows[270], rows[299] = pool[0], pool[0], pool[0], pool[0]      # a row four times, in both tiles
    td[0], td[5], td[270], td[299] = 0.5, -7.0, 2.0, 7.0                   # |-7| and 7 tie: one value either way
    rows[10], rows[11], rows[280] = pool[1], pool[1], pool[1]
    td[10], td[11], td[280] = np.nan, 0.25, 0.125                          # NaN stands for the old max_priority 2.5 and wins
    rows[20], rows[21] = pool[2], pool[2]
    td[20], td[21] = np.inf, -np.inf
    rows[30], rows[31], rows[32], rows[33] = -1, n, 2 ** 40, -2 ** 40
    td[30:34] = 1e6                                                        # skipped: they must not raise max_priority
    rows[40], rows[41] = zero_rows[0], zero_rows[zero_rows >= 2 * BLK][0]
    td[40:42] = 1e6
    rows[50], td[50] = n - 2, 50.0                                         # a row of the ragged last block: the largest finite priority
    assert mass[n - 2] > 0
    m, bm, bmin = _structure(mass)
    mp = torch.full((1,), 2.5, dtype=torch.float32, device=DEV)
    before = [t.clone() for t in (m, bm, bmin)]
    P.per_update(m, bm, bmin, mp, _dev(rows), _dev(td), alpha, eps)
    want, want_mp, written = PC.update_reference(mass, 2.5, rows, td, alpha, eps)
    got = m.double().cpu().numpy()
    untouched = np.setdiff1d(np.arange(n), written)
    assert np.array_equal(got[untouched], mass.astype(np.float64)[untouched]), "a row that was not named, or was skipped, changed"
    assert (got[zero_rows] == 0).all() and (got[pos_rows] > 0).all() and np.isfinite(got).all()
    err = np.abs(got[written] - want[written]) / want[written]
    print(f"[per_update] {len(written)} rows written; masses: largest relative error {err.max() / REL:.3f} of the bound {REL:.2e}")
    assert err.max() <= REL
    for r, p in ((pool[0], np.float64(F32(7.0) + eps)), (pool[1], 2.5), (pool[2], 2.5)):
        assert abs(got[r] / p ** 0.6 - 1) <= REL, (r, got[r], p ** 0.6)
    assert mp.item() == float(want_mp) == float(F32(50.0) + eps)
    full_bm, full_bmin = P.per_refresh(m)
    assert torch.equal(bm, full_bm) and torch.equal(bmin, full_bmin), "touched blocks differ from a full refresh"
    assert torch.equal(bm[1], before[1][1]) and torch.equal(bmin[1], before[2][1]) and not torch.equal(bm[0], before[1][0])
    # two runs; (B, 1) td; max_priority never decreases
    m2, bm2, bmin2 = _structure(mass)
    mp2 = torch.full((1,), 2.5, dtype=torch.float32, device=DEV)
    P.per_update(m2, bm2, bmin2, mp2, _dev(rows), _dev(td).reshape(-1, 1), alpha, eps)
    assert not MG.differing([m, bm, bmin, mp], [m2, bm2, bmin2, mp2])
    P.per_update(m2, bm2, bmin2, mp2, _dev(rows[:1]), _dev(np.array([0.5], dtype=F32)), alpha, eps)
    assert mp2.item() == mp.item()
    with pytest.raises(ValueError, match=r"td must be a contiguous float32 tensor of shape \(300,\) or \(300, 1\)"):
        P.per_update(m, bm, bmin, mp, _dev(rows), _dev(td[:-1]), alpha, eps)
    with pytest.raises(ValueError, match="max_priority must be a contiguous float32 tensor of 1 value"):
        P.per_update(m, bm, bmin, torch.ones(2, device=DEV), _dev(rows), _dev(td), alpha, eps)
    with pytest.raises(ValueError, match=r"beta=1.5 must be a number in \[0, 1\]"):
        P.per_sample(m, bm, bmin, _dev(td).abs(), 1.5)
    with pytest.raises(ValueError, match="block_mass must be a contiguous float32 tensor of 4 value"):
        P.per_sample(m, bm[:3], bmin, _dev(td))


# ---- 4. the buffer
CFG = ((8, 8), (4, 4), 1, (np.uint8, F32))
MODES = {"stacked": {}, "frame_dedup": dict(frame_dedup=True), "single_store": dict(optimize_memory_usage=True),
         "single_store_frame_dedup": dict(optimize_memory_usage=True, frame_dedup=True)}


def _buffer(fs, timeouts, **kw):
    image_hw, tactile_hw, Sn, dtypes = CFG
    shapes = {"image": (fs,) + image_hw + (3,), "tactile": (fs, 3 * Sn) + tactile_hw}
    return m3l_amd.DeviceReplayBuffer(T * E, E, shapes, {"image": dtypes[0], "tactile": dtypes[1]}, A, handle_timeout_termination=timeouts,
                                      device=DEV, **kw)


def _add(buf, st, k):
    buf.add({key: v[k] for key, v in st["obs"].items()}, {key: v[k] for key, v in st["next_obs"].items()}, st["actions"][k], st["rewards"][k],
            st["dones"][k], st["infos"][k])


def _check_structure(buf, model, what):
    mass = buf.mass.cpu().numpy()
    valid = sorted(model.valid_steps())
    first, count = buf._valid_steps()
    assert valid == sorted((first + i) % T for i in range(count)), what
    inside = np.zeros(T, dtype=bool)
    inside[valid] = True
    assert (mass[~inside] == 0).all(), f"{what}: mass outside the valid steps {valid}: {mass}"
    assert (mass[inside] > 0).all() and np.isfinite(mass).all(), f"{what}: zero mass inside the valid steps {valid}: {mass}"
    bm, bmin = P.per_refresh(buf.mass)
    assert torch.equal(bm, buf.block_mass) and torch.equal(bmin, buf.block_min), what
    return mass


@pytest.mark.parametrize("n_steps", [1, 3])
@pytest.mark.parametrize("mode", sorted(MODES))
def test_buffer_on_the_nstep_stream(mode, n_steps):
    kw = MODES[mode]
    single, dedup = bool(kw.get("optimize_memory_usage")), bool(kw.get("frame_dedup"))
    if single and n_steps > 1:
        with pytest.raises(ValueError, match="n_steps > 1 needs optimize_memory_usage=False"):
            _buffer(2, False, prioritized=True, n_steps=n_steps, **kw)
        return
    fs, timeouts, gamma, alpha, beta = 2, not single, 0.97, 0.6, 0.4
    st = NC.make_stream(fs, CFG[0], CFG[1], CFG[2], CFG[3][0], CFG[3][1], seed=31)
    plain = _buffer(fs, timeouts, n_steps=n_steps, gamma=gamma, **kw)
    per = _buffer(fs, timeouts, n_steps=n_steps, gamma=gamma, prioritized=True, alpha=alpha, beta=beta, **kw)
    twin = _buffer(fs, timeouts, n_steps=n_steps, gamma=gamma, prioritized=True, alpha=alpha, beta=beta, **kw)
    assert plain.mass is None and per.store_bytes()["scalars"] == plain.store_bytes()["scalars"] + 4 * (T * E + 2 + 1)
    env = NC.RewardNorm()
    g = np.random.default_rng(5)
    for k in range(max(NC.CHECKPOINTS)):
        for buf in (plain, per, twin):
            _add(buf, st, k)
        smodel, fmodel = FC.fill_models(k + 1, T, fs, single, st)
        model = fmodel if dedup else smodel
        what = f"{mode} n_steps={n_steps} after {k + 1} adds"
        mass = _check_structure(per, model, what)                      # after every add()
        if k + 1 not in NC.CHECKPOINTS:
            continue
        valid = set(model.valid_steps())
        u = g.random(16).astype(F32)
        u[0] = 0.0
        batch = per.sample(16, env=env, u=_dev(u))
        assert isinstance(batch, m3l_amd.PrioritizedReplayBatch) and batch.weights.shape == (16, 1), what
        rows = batch.rows.cpu().numpy()
        assert set((rows // E).tolist()) <= valid, f"{what}: rows {rows} outside the valid steps {sorted(valid)}"
        _follows(what, mass.ravel(), u, batch.rows, batch.weights, beta)
        # every field but weights: the plain buffer's sample of the same rows, bit for bit
        base = plain.sample(1, env=env, indices=(rows // E, rows % E))
        for name in base._fields:
            assert not MG.differing(getattr(batch, name), getattr(base, name)), f"{what}: {name} differs from the plain buffer"
        if n_steps == 1:
            assert torch.equal(batch.next_rows, batch.rows) and (batch.discounts == float(F32(gamma))).all() and batch.discounts.shape == (16, 1)
        # indices=: those rows, and their weights
        given = per.sample(1, env=env, indices=(rows // E, rows % E), beta=1.0)
        assert torch.equal(given.rows, batch.rows) and not MG.differing(list(given[:-1]), list(batch[:-1]))
        want = PC.weights_reference(mass, rows, 1.0)
        assert (np.abs(given.weights.double().cpu().numpy() - want) / want).max() <= REL, what
        # a drawn batch (torch.rand): valid rows only
        drawn = per.sample(64).rows.cpu().numpy()
        assert set((drawn // E).tolist()) <= valid, what
        # update_priorities, then the next sample follows the restatement on the new masses; the twin gives the same bits
        td = (g.standard_normal(16) * 2).astype(F32)
        td[3] = np.nan
        old_mp = per.max_priority.item()
        for buf in (per, twin):
            assert not MG.differing(list(buf.sample(16, env=env, u=_dev(u))), list(batch)), what
            buf.update_priorities(batch.rows, _dev(td).reshape(-1, 1))
        want_mass, want_mp, written = PC.update_reference(mass, old_mp, rows, td, alpha, per.priority_eps)
        mass = _check_structure(per, model, what + " after update_priorities")
        assert (np.abs(mass.ravel().astype(np.float64) - want_mass)[written] <= REL * want_mass[written]).all() and per.max_priority.item() == float(want_mp)
        u2 = g.random(8).astype(F32)
        after = per.sample(8, u=_dev(u2), beta=0.9)
        _follows(what + " after update_priorities", mass.ravel(), u2, after.rows, after.weights, 0.9)
        assert not MG.differing(list(after), list(twin.sample(8, u=_dev(u2), beta=0.9))), what
    assert per.full and per.pos == 3
    per.reset()
    assert (per.mass == 0).all() and (per.block_mass == 0).all() and torch.isinf(per.block_min).all() and per.max_priority.item() == 1.0
    with pytest.raises(ValueError, match="the buffer is empty"):
        per.sample(4)
    with pytest.raises(ValueError, match="belong to prioritized=True"):
        plain.sample(4, beta=0.5)
    with pytest.raises(ValueError, match="indices and u both name the rows"):
        twin.sample(4, indices=([3], [0]), u=_dev(u))


# ---- 5. the weighted critic loss
@pytest.mark.parametrize("B", [5, 300])
def test_weighted_critic_loss(B):
    g = np.random.default_rng(B)
    q, t = g.standard_normal((2, B)).astype(F32) * 3, g.standard_normal(B).astype(F32) * 3
    w = g.uniform(0.05, 1.0, B).astype(F32)
    d = q.astype(np.float64) - t.astype(np.float64)
    ref_loss = 0.5 * (w * d * d).mean(axis=1).sum()
    ref_dq, ref_td = 1.7 * w * d / B, 0.5 * np.abs(d).sum(axis=0)

    def run(weights, td_errors=True, scale=1.7):
        qd = _dev(q).requires_grad_()
        out = S.critic_loss_from(qd, _dev(t), weights, td_errors)
        loss, td = out if td_errors else (out, None)
        (loss * scale).backward()
        return loss.detach(), qd.grad, td
    loss, dq, td = run(_dev(w).reshape(B, 1))
    errs = (abs(loss.item() - ref_loss) / max(1.0, abs(ref_loss)), float(np.abs(dq.double().cpu().numpy() - ref_dq).max() / np.abs(ref_dq).max()),
            float((np.abs(td.double().cpu().numpy() - ref_td) / np.maximum(1.0, ref_td)).max()))
    print(f"[weighted critic loss B={B}] loss err {errs[0]:.2e}, gradient err {errs[1]:.2e} of the largest entry, td err {errs[2]:.2e} (bound {SAC_TOL:.0e})")
    assert loss.dim() == 0 and td.shape == (B,) and not td.requires_grad and max(errs) <= SAC_TOL
    assert not MG.differing([loss, dq, td], list(run(_dev(w))))                                        # two runs, (B,) weights
    plain = run(None, td_errors=False)                                                                # the existing entry
    ones = run(torch.ones(B, device=DEV))
    none_td = run(None)
    assert torch.equal(ones[0], plain[0]) and torch.equal(ones[1], plain[1]), "weights of ones differ from the unweighted loss"
    assert torch.equal(none_td[0], plain[0]) and torch.equal(none_td[1], plain[1]) and torch.equal(none_td[2], ones[2])
    only_loss = run(_dev(w), td_errors=False)
    assert torch.equal(only_loss[0], loss) and torch.equal(only_loss[1], dq)
    with pytest.raises(ValueError, match=r"weights: a float32 tensor of shape"):
        S.critic_loss_from(_dev(q), _dev(t), _dev(w)[:-1])


# ---- 6. the memory contract of every new entry
def test_memory_contract_of_the_per_entry_points(monkeypatch):
    fs = 2
    st = NC.make_stream(fs, CFG[0], CFG[1], CFG[2], CFG[3][0], CFG[3][1], seed=77)
    bufs = [_buffer(fs, True, prioritized=True, n_steps=n, **kw) for n, kw in ((1, {}), (3, dict(frame_dedup=True)))]
    for k in range(17):
        for buf in bufs:
            _add(buf, st, k)
    big, small = PC.general_mass(PC.N_BIG, seed=9), PC.general_mass(PC.N_SMALL, seed=9)
    g = np.random.default_rng(12)
    u = {n: _dev(g.random(n).astype(F32)) for n in (7, 16, 300)}
    q, t, w = (_dev(g.standard_normal(s).astype(F32)) for s in ((2, 300), (300,), (300,)))
    rows_up = _dev(g.integers(-2, PC.N_BIG + 2, 300).astype(np.int64))
    td_up = _dev(g.standard_normal(300).astype(F32))

    def work(gd):
        out = {}
        for name, mass in (("big", big), ("small", small)):
            m = _dev(mass)
            bm, bmin = P.per_refresh(m)
            out[name] = [bm, bmin] + [list(P.per_sample(m, bm, bmin, u[B], 0.4, s)) for B in (7, 300) for s in (True, False)]
            gd.check(f"after per_sample of {name}")
            if name == "big":
                mp = torch.ones(1, device=DEV)
                P.per_update(m, bm, bmin, mp, rows_up, td_up, 0.6, 1e-6)
                drawn = P.per_sample(m, bm, bmin, u[300], 0.4)[0]
                out["updated"] = [m, bm, bmin, mp, list(P.per_sample(m, bm, bmin, None, 0.4, rows=drawn))]
                gd.check("after per_update")
        for i, buf in enumerate(bufs):
            b = buf.sample(16, u=u[16])
            out[f"buf{i}"] = [dict(b.observations), dict(b.next_observations)] + list(b[1:2]) + list(b[3:])
            gd.check(f"after the sample of buffer {i}")
        # a buffer allocated and filled under the guard (m3l_replay_per_add): the slots never written hold the fill, and no sample reaches them
        for i, kw in enumerate((dict(frame_dedup=True), dict(optimize_memory_usage=True))):
            fresh = _buffer(fs, not kw.get("optimize_memory_usage", False), prioritized=True, **kw)
            for k in range(5 + 4 * i):
                _add(fresh, st, k)
            b = fresh.sample(16, u=u[16])
            fresh.update_priorities(b.rows, td_up[:16])
            b2 = fresh.sample(16, u=u[16])
            out[f"fresh{i}"] = [dict(b.observations), dict(b.next_observations), dict(b2.observations)] + list(b[3:]) + list(b2[3:]) + [fresh.block_mass, fresh.block_min]
            gd.check(f"after the adds and samples of fresh buffer {i}")
        qd = q.clone().requires_grad_()
        loss, td = S.critic_loss_from(qd, t, w.abs(), True)
        loss.backward()
        out["sac"] = [loss.detach(), td, qd.grad]
        gd.check("after the weighted critic loss")
        return out
    MG.run_contract(monkeypatch, work, need_ws=False)
