"""Inputs and the float64 yardstick of the KoLeo tests (test_koleo_cpu.py, test_koleo_gpu.py, golden/make_golden_koleo.py).

  koleo_f64(x)     the formulas of include/m3l_amd.h ("KoLeo regulariser") in float64, the gradient from its closed form (no autograd):
                   y_i = x_i / max(||x_i||, eps), I(i) = argmax_{j != i} y_i . y_j (lowest j on an exact tie; a single row is its own
                   neighbour), d_i = ||y_i - y_I(i) + 1e-8||, loss = -(1/n) sum_i log(d_i + eps);
                   g_i = -1 / (n (d_i + eps)), u_i = (y_i - y_I(i) + 1e-8) / d_i, dy_j = g_j u_j - sum_{i : I(i) = j} g_i u_i,
                   dx_j = (dy_j - y_j (y_j . dy_j)) / ||x_j||, or dy_j / eps where the norm was clamped
  neighbour_gap(x) the condition every test input satisfies: in float64 every row's best product is at least GAP above every product that is
                   not exactly equal to it, and products exactly equal to the best come from identical rows or belong to a zero row (ties in
                   any arithmetic).  Returns the smallest gap.
  random_rows / planted_rows   the constructions of the inputs."""
import numpy as np
import torch

GAP = 1e-4
PD_EPS = 1e-8

RANDOM_SHAPES = [(35, 256), (64, 192), (67, 100), (33, 50)]
PLANTED_SHAPES = [(130, 256), (300, 192), (300, 256), (512, 384), (1030, 256), (4096, 384)]


def random_rows(n, D, seed=0):
    return torch.randn(n, D, generator=torch.Generator().manual_seed(seed))


def planted_rows(n, D, seed=0):
    """ceil(n / 3) random unit anchors, each with a child at distance 0.1 and a child at distance 0.2 in random directions orthogonal to it;
    the far children of the last anchors are left out when n is no multiple of 3; rows scaled by 0.25 .. 4.25 and permuted.  An anchor's
    neighbour is its near child, both children's neighbour is the anchor: anchors have in-degree 2 (1 without a far child), near children
    1, far children 0.  -> (rows float32, kind int64: 0 anchor, 1 near child, 2 far child)."""
    g = torch.Generator().manual_seed(seed)
    m = -(-n // 3)
    a = torch.nn.functional.normalize(torch.randn(m, D, generator=g, dtype=torch.float64), dim=-1)

    def orth():
        o = torch.randn(m, D, generator=g, dtype=torch.float64)
        o = o - (o * a).sum(-1, keepdim=True) * a
        return torch.nn.functional.normalize(o, dim=-1)
    rows = torch.cat([a, a + 0.1 * orth(), a + 0.2 * orth()])[:n]
    kind = torch.cat([torch.zeros(m), torch.ones(m), 2 * torch.ones(m)]).long()[:n]
    rows = rows * (0.25 + 4.0 * torch.rand(n, 1, generator=g, dtype=torch.float64))
    perm = torch.randperm(n, generator=g)
    return rows[perm].float(), kind[perm]


def _normalized(x, eps):
    norm = np.sqrt((x * x).sum(-1))
    return x / np.maximum(norm, eps)[:, None], norm


def _products(y):
    dots = y @ y.T
    np.fill_diagonal(dots, -np.inf)
    return dots


def koleo_f64(x, eps=1e-8):
    """x (n, D) array-like -> dict(loss, grad (n, D), indices (n,) int64, dist (n,)) in float64."""
    x = np.asarray(x, dtype=np.float64)
    n = x.shape[0]
    y, norm = _normalized(x, eps)
    idx = np.argmax(_products(y), axis=1).astype(np.int64) if n > 1 else np.zeros(1, dtype=np.int64)      # argmax: the first of equal values
    diff = y - y[idx] + PD_EPS
    d = np.sqrt((diff * diff).sum(-1))
    loss = -np.log(d + eps).mean()
    gu = (-1.0 / (n * (d + eps)) / d)[:, None] * diff
    dy = gu.copy()
    np.subtract.at(dy, idx, gu)
    clamped = norm < eps
    safe = np.where(clamped, 1.0, norm)
    dx = (dy - y * (y * dy).sum(-1, keepdims=True)) / safe[:, None]
    dx[clamped] = dy[clamped] / eps
    return dict(loss=float(loss), grad=dx, indices=idx, dist=d)


def neighbour_gap(x, eps=1e-8):
    """Asserts the condition of the module docstring and returns the smallest gap (inf when every row's candidates are all tied)."""
    x = np.asarray(x, dtype=np.float64)
    n = x.shape[0]
    if n < 3:
        return float("inf")
    y, _ = _normalized(x, eps)
    dots = _products(y)
    best = dots.max(axis=1)
    tied = dots == best[:, None]
    gap = np.where(tied, np.inf, best[:, None] - dots).min(axis=1)
    for i in np.nonzero(tied.sum(axis=1) > 1)[0]:
        js = np.nonzero(tied[i])[0]
        assert not y[i].any() or all(np.array_equal(x[j], x[js[0]]) for j in js), f"row {i}: equal products of rows that are not identical"
    assert float(gap.min()) >= GAP, f"smallest gap {gap.min():.3e} below {GAP}"
    return float(gap.min())


def in_degree(indices):
    indices = np.asarray(indices)
    return np.bincount(indices, minlength=indices.shape[0])


# every input the GPU tests build beyond the recorded cases: name -> (kind, n, D, one seed per group)
GPU_INPUTS = {
    "planted_300x192": ("planted", 300, 192, (0,)), "planted_512x384": ("planted", 512, 384, (0,)), "planted_1030x256": ("planted", 1030, 256, (0,)),
    "planted_4096x384": ("planted", 4096, 384, (0,)), "randn_2x35x256": ("randn", 35, 256, (0, 1)), "planted_2x300x256": ("planted", 300, 256, (0, 1)),
    "contract_2x35x192": ("randn", 35, 192, (0, 1)), "contract_1x130x50": ("randn", 130, 50, (0,)),
}


def gpu_input(name):
    """-> list of the groups' (n, D) float32 tensors."""
    kind, n, D, seeds = GPU_INPUTS[name]
    return [planted_rows(n, D, s)[0] if kind == "planted" else random_rows(n, D, s) for s in seeds]
