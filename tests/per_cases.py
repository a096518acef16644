"""Prioritised replay of DeviceReplayBuffer(prioritized=True) restated in numpy / float64 (test_replay_per_cpu.py, test_replay_per_gpu.py).

Neither the reference tree nor SB3 has prioritised replay: the rule (Schaul et al. 2016, proportional variant) is restated from
include/m3l_amd.h ("prioritised replay") and nothing pins the restatement (parity unpinned); the cases written out by hand in
test_replay_per_cpu.py hold it.

mass (N) >= 0, blocks of PER_BLOCK rows, C the inclusive prefix of mass and Cb that of the block sums, all float64:
  1. total = the sum of the block sums
  2. x_k = (k + u_k) * (total / B) if stratified, else u_k * total
  3. block j = the smallest j with Cb[j] > x_k
  4. residual = x_k - Cb[j - 1]  (0 in front of block 0)
  5. leaf i = the smallest i of block j whose inclusive prefix within the block exceeds the residual
  where there is no such leaf, or no such block (x_k >= total): the last leaf, or block, of positive mass
  weights = (the smallest positive mass / mass[row])^beta
In float64 the prefix grows at positive entries only, so the row found always has positive mass; the kernel adds "mass > 0" to 3 and 5 for the
same end under float32 rounding.  `sample_reference` walks the two levels as the rule states them; `flat_row` is the one-level search over C
that they must agree with.

update: priority = |td| + eps (float32 sum, as the kernel forms it), a non-finite td -> the old max_priority; a row outside [0, N) or of zero mass
is skipped; of duplicates the largest priority wins; mass = priority^alpha in float64; max_priority = max(itself, the finite priorities applied)."""
import numpy as np

from m3l_amd.replay import PER_BLOCK

F32 = np.float32


def blocks_of(n):
    return (n + PER_BLOCK - 1) // PER_BLOCK


def refresh_reference(mass):
    """mass (N) -> (block_mass, block_min) (nb) float64: the sum and the smallest positive leaf (+inf: none) of every block."""
    m = np.asarray(mass, dtype=np.float64).ravel()
    nb = blocks_of(m.size)
    bm, bmin = np.zeros(nb), np.full(nb, np.inf)
    for j in range(nb):
        leaves = m[j * PER_BLOCK:(j + 1) * PER_BLOCK]
        bm[j] = leaves.sum()
        if (leaves > 0).any():
            bmin[j] = leaves[leaves > 0].min()
    return bm, bmin


def targets(total, u, stratified=True):
    """x_k in float64 from the float32 u."""
    u = np.asarray(u, dtype=np.float64)
    B = u.size
    return (np.arange(B) + u) * (total / B) if stratified else u * total


def flat_row(mass, x):
    """The smallest row whose inclusive prefix exceeds x, else the last row of positive mass."""
    m = np.asarray(mass, dtype=np.float64).ravel()
    C = np.cumsum(m)
    r = int(np.searchsorted(C, x, side="right"))
    return r if r < m.size else int(np.flatnonzero(m > 0)[-1])


def sample_reference(mass, u, beta, stratified=True):
    """mass (N) float32 with at least one positive entry, u (B) float32 -> dict(rows (B) int64, weights (B, 1) float64, x (B) float64,
    total, C (N) float64 inclusive prefix of mass)."""
    m = np.asarray(mass, dtype=np.float64).ravel()
    assert (m >= 0).all() and (m > 0).any()
    bm, bmin = refresh_reference(m)
    Cb = np.cumsum(bm)
    total = Cb[-1]
    x = targets(total, u, stratified)
    rows = []
    for xk in x:
        hit = np.flatnonzero(Cb > xk)
        j = int(hit[0]) if hit.size else int(np.flatnonzero(bm > 0)[-1])
        res = xk - (Cb[j - 1] if j > 0 else 0.0)
        leaves = m[j * PER_BLOCK:(j + 1) * PER_BLOCK]
        hit = np.flatnonzero(np.cumsum(leaves) > res)
        i = int(hit[0]) if hit.size else int(np.flatnonzero(leaves > 0)[-1])
        rows.append(j * PER_BLOCK + i)
    rows = np.asarray(rows, dtype=np.int64)
    assert (m[rows] > 0).all()
    weights = (bmin.min() / m[rows]) ** np.float64(beta)
    return dict(rows=rows, weights=weights.reshape(-1, 1), x=x, total=total, C=np.cumsum(m))


def weights_reference(mass, rows, beta):
    m = np.asarray(mass, dtype=np.float64).ravel()
    return ((m[m > 0].min() / m[np.asarray(rows)]) ** np.float64(beta)).reshape(-1, 1)


def update_reference(mass, max_priority, rows, td, alpha, eps):
    """-> (mass (N) float64 after the update, max_priority after it, the rows written).  td and eps are float32; the priority |td| + eps is the
    float32 sum the kernel forms, its power is float64."""
    m = np.asarray(mass, dtype=np.float64).ravel().copy()
    old = F32(max_priority)
    best, new_max = {}, old
    for r, t in zip(np.asarray(rows).tolist(), np.asarray(td, dtype=F32).ravel()):
        if r < 0 or r >= m.size or m[r] == 0:
            continue
        p = F32(abs(t)) + F32(eps) if np.isfinite(t) else old
        if np.isfinite(t):
            new_max = max(new_max, p)
        best[r] = max(best.get(r, p), p)
    for r, p in best.items():
        m[r] = np.float64(p) ** np.float64(alpha)
    return m, F32(new_max), sorted(best)


# ---- the inputs of the exact-arithmetic check: integer leaves in [0, 8], B a power of two that divides total, u multiples of 2^-8
N_BIG, N_SMALL = 3 * PER_BLOCK + 5, 5
N_MANY = 257 * PER_BLOCK + 3          # 258 blocks: more than the 256 threads that form the block prefix, so a thread sums a chunk of two


def _u(B, seed):
    g = np.random.default_rng(seed)
    u = (g.integers(0, 256, B) / 256.0).astype(F32)
    u[::3] = 0.0                       # targets exactly on the boundaries k total / B
    return u


def _fit(m, total):
    """Raise or lower positive leaves, kept within [1, 8], until the mass sums to `total`: the zeros stay where they are."""
    m = m.copy()
    for i in np.flatnonzero(m > 0):
        d = total - int(m.sum())
        if d == 0:
            break
        m[i] += min(8 - m[i], d) if d > 0 else -min(m[i] - 1, -d)
    assert m.sum() == total and m.max() <= 8 and m.min() >= 0, (m.sum(), total)
    return m


def _aim(u, q, value):
    """Set one u so that its target (k + u_k) * q is the integer `value` exactly (q a power of two up to 256, so u_k is a multiple of 2^-8)."""
    k = value // q
    assert 0 <= k < u.size and 256 % q == 0
    u[k] = F32((value % q) / q)


def exact_cases():
    """name -> (mass (N) float32 of integers, u (B) float32).  In the two large cases total / B = 32, and targets are aimed at the end of block 0 —
    in the first case that is also the end of the zero block 1, so the row is the first positive leaf of block 2 behind its zero run — at the
    last row's prefix minus its mass and at a leaf prefix in front of a zero run."""
    g = np.random.default_rng(11)
    out = {}
    # a zero block in the middle, zero runs across the other block edges
    m = g.integers(0, 9, N_BIG).astype(np.int64)
    m[PER_BLOCK:2 * PER_BLOCK] = 0
    m[PER_BLOCK - 7:PER_BLOCK] = 0
    m[2 * PER_BLOCK:2 * PER_BLOCK + 9] = 0
    m[3 * PER_BLOCK - 3:3 * PER_BLOCK + 2] = 0
    m[40:60] = 0
    m, u = _fit(m, 256 * 32), _u(256, 1)
    C = np.cumsum(m)
    for value in (C[PER_BLOCK - 1], C[39], C[3 * PER_BLOCK - 4], C[-1] - m[-1]):
        _aim(u, 32, int(value))
    out["zero_block_in_the_middle"] = (m, u)
    # one leaf in 8: zero runs everywhere, the ragged last block in use
    m = np.zeros(N_BIG, dtype=np.int64)
    m[::8] = g.integers(1, 9, m[::8].size)
    m[N_BIG - 1] = 3
    m, u = _fit(m, 64 * 32), _u(64, 2)
    C = np.cumsum(m)
    for value in (C[PER_BLOCK - 1], C[2 * PER_BLOCK - 1], C[8], C[-1] - m[-1]):
        _aim(u, 32, int(value))
    out["sparse"] = (m, u)
    for name, n in (("big", N_BIG), ("small", N_SMALL)):
        m = np.zeros(n, dtype=np.int64)
        m[-1] = 8
        out[f"all_mass_in_the_last_leaf_{name}"] = (m, _u(8, 3))
        m = np.zeros(n, dtype=np.int64)
        m[0] = 8
        out[f"all_mass_in_the_first_leaf_{name}"] = (m, _u(4, 4))
    out["five_rows"] = (np.array([2, 0, 0, 5, 1], dtype=np.int64), _u(8, 5))
    # 258 blocks, one leaf in 32, blocks 100 and 101 empty; total / B = 128, a power of two: the product (k + u) * 128 is exact.  Targets on the
    # end of block 1 (between the chunks of two threads), of block 127 (between two waves), of block 99 (= of the empty blocks), of the ring
    m = np.zeros(N_MANY, dtype=np.int64)
    m[::32] = g.integers(1, 9, m[::32].size)
    m[100 * PER_BLOCK:102 * PER_BLOCK] = 0
    m[N_MANY - 1] = 5
    m, u = _fit(m, 256 * 128), _u(256, 6)
    C = np.cumsum(m)
    for value in (C[2 * PER_BLOCK - 1], C[128 * PER_BLOCK - 1], C[100 * PER_BLOCK - 1], C[-1] - m[-1], C[32]):
        _aim(u, 128, int(value))
    out["many_blocks"] = (m, u)
    return {k: (m.astype(F32), u) for k, (m, u) in out.items()}


def boundary_hits(mass, u):
    """How many targets of an exact case fall exactly on (a leaf prefix, a block prefix)."""
    ref = sample_reference(mass, u, 0.5)
    bm, _ = refresh_reference(mass)
    return int(np.isin(ref["x"], ref["C"]).sum()), int(np.isin(ref["x"], np.cumsum(bm)).sum())


def general_mass(n, seed):
    """Positive masses spread log-uniformly over [1e-3, 1e3] — the extremes are set, a ratio of 10^6 — with a fifth of the rows and one run across
    a block edge zero."""
    g = np.random.default_rng(seed)
    m = np.exp(g.uniform(np.log(1e-3), np.log(1e3), n))
    m[g.random(n) < 0.2] = 0
    if n > PER_BLOCK:
        m[PER_BLOCK - 20:PER_BLOCK + 30] = 0
    m[1], m[n - 2] = 1e-3, 1e3
    return m.astype(F32)
