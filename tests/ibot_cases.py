"""Inputs and the float64 yardstick of the iBOT patch-loss tests (test_ibot_cpu.py, test_ibot_gpu.py, golden/make_golden_ibot.py).

  inputs(Q, R, K)   student and teacher logits (Q, R, K) float32 — cosines of random unit rows against random prototype directions scaled by
                    0.5 .. 1.5, what the weight-normalised prototype layer gives, |l| <= 1.5 — and a non-zero centre (K,) float32, all seeded
  ibot_f64(...)     the formulas of include/m3l_amd.h ("iBOT patch loss") in float64, the gradient from its closed form (no autograd):
                    tsum[r,k] = sum_q softmax((T[q,r,:] - c) / tt)[k];  loss = 1/R sum_r (Q sum_p lse(S[p,r,:] / ts) - 1/ts sum_k tsum[r,k] sum_p S[p,r,k]);
                    dS[p,r,k] = 1 / (ts R) (Q softmax(S[p,r,:] / ts)[k] - tsum[r,k]);  pending = sum over rows of T / n;
                    centre' = c m + pending / (Q R / n) (1 - m)
  sinkhorn_f64(...) the Sinkhorn-Knopp targets over all Q R rows in the log domain (the restatement test_sinkhorn_cpu.py pins to the reference)
  sample_rows(R)    the rows of every view whose dS and probabilities the fixture stores in full (the complete float64 arrays of a case are 4 to
                    80 MB, a committed file holds 1 MiB); every other row enters through the recorded column sums and row norms."""
import hashlib

import numpy as np
import torch
import torch.nn.functional as F

STUDENT_TEMP, TEACHER_TEMP, MOMENTUM = 0.1, 0.05, 0.9
# (Q, R, K) -> n, the patches per sample (R = B n) of the recorded centre update
RECORDED = {(1, 5, 1000): 5, (2, 257, 1000): 257, (3, 70, 1000): 7, (2, 300, 4096): 12}
GPU_ONLY = {(2, 1030, 1000): 103, (2, 35, 65536): 5}
SHAPES = {**RECORDED, **GPU_ONLY}


def case_name(Q, R, K):
    return f"q{Q}_r{R}_k{K}"


def cosine_logits(rows, K, seed, dim=32):
    g = torch.Generator().manual_seed(seed)
    x = F.normalize(torch.randn(rows, dim, generator=g), dim=-1)
    W = F.normalize(torch.randn(K, dim, generator=g), dim=-1) * (0.5 + torch.rand(K, 1, generator=g))
    return x @ W.t()


def inputs(Q, R, K):
    """-> S (Q, R, K), T (Q, R, K), centre (K,), float32 CPU tensors."""
    S = cosine_logits(Q * R, K, seed=10_000 + 7 * Q + 3 * R + K).view(Q, R, K)
    T = cosine_logits(Q * R, K, seed=20_000 + 7 * Q + 3 * R + K).view(Q, R, K)
    c = 0.1 * torch.randn(K, generator=torch.Generator().manual_seed(30_000 + K))
    return S, T, c


def digest(*tensors):
    h = hashlib.sha256()
    for t in tensors:
        h.update(np.ascontiguousarray(t.numpy() if isinstance(t, torch.Tensor) else t).tobytes())
    return h.hexdigest()


def _lse(z):
    m = z.max(axis=-1, keepdims=True)
    return m + np.log(np.exp(z - m).sum(axis=-1, keepdims=True))


def ibot_f64(S, T, center, n, ts=STUDENT_TEMP, tt=TEACHER_TEMP, momentum=MOMENTUM):
    """-> dict(loss, dS (Q, R, K), probs (Q, R, K), tsum (R, K), pending (K,), center_after (K,)) in float64.  `center` is the K-vector in the
    centre's place (the centre, or the Sinkhorn-Knopp vector)."""
    S, T, c = (np.asarray(a, dtype=np.float64) for a in (S, T, center))
    Q, R, K = S.shape
    zs = S / ts
    lse_s = _lse(zs)
    zt = (T - c) / tt
    probs = np.exp(zt - _lse(zt))
    tsum = probs.sum(axis=0)
    loss = (Q * lse_s.sum() - (tsum * S.sum(axis=0)).sum() / ts) / R
    dS = (Q * np.exp(zs - lse_s) - tsum[None]) / (ts * R)
    pending = T.reshape(-1, K).sum(axis=0) / n
    center_after = c * momentum + pending / (Q * R // n) * (1 - momentum)
    return dict(loss=float(loss), dS=dS, probs=probs, tsum=tsum, pending=pending, center_after=center_after)


def sinkhorn_f64(T, tt=TEACHER_TEMP, n_iterations=3):
    """-> (probabilities (rows, K), the K-vector tt u) over all rows of T, float64."""
    z = np.asarray(T, dtype=np.float64).reshape(-1, np.shape(T)[-1]) / tt
    w = np.zeros(z.shape[0])
    u = None
    for _ in range(n_iterations):
        u = _lse((z - w[:, None]).T)[:, 0]
        w = _lse(z - u[None, :])[:, 0]
    return np.exp(z - u[None, :] - w[:, None]), tt * u


def sample_rows(R):
    return sorted({0, R // 2, R - 1})


def summaries(a):
    """What the fixture keeps of a (Q, R, K) array besides the sampled rows: column sums (Q, K), row 2-norms (Q, R), the largest magnitude."""
    a = np.asarray(a, dtype=np.float64)
    return dict(colsum=a.sum(axis=1), rownorm=np.sqrt((a * a).sum(axis=2)), amax=np.float64(np.abs(a).max()))
