"""CPU-only checks of the Sinkhorn-Knopp teacher assignment: the float64 yardstick of the GPU tests against the results recorded from the
reference's own DINOLoss.sinkhorn_knopp_teacher (tests/golden/make_golden_sinkhorn.py), the public surface (methods, the VTDINO keyword,
argument checks), and the rank-order gather of the column pairs under a two-process gloo group.  No kernel is launched here."""
import os
import socket

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

import m3l_amd
from m3l_amd import _lib as L
from m3l_amd import dino as D
from test_vtdino_cpu import _z, build_step_module

SK_SYMBOLS = ["m3l_op_sk_row_splits", "m3l_op_sk_ws_bytes", "m3l_op_sk_colstats", "m3l_op_sk_colcombine", "m3l_op_sk_probs"]


def sinkhorn_log_domain(logits, teacher_temp, n_iterations=3, dtype=torch.float64):
    """The iteration in the log domain: z = L / tt, w = 0; n times u[k] = logsumexp_r(z[r,k] - w[r]), w[r] = logsumexp_k(z[r,k] - u[k]);
    T = exp(z - u - w).  logits (rows, K) -> (T, tt * u): the probabilities and the vector that stands in the centre's place."""
    z = logits.to(dtype) / teacher_temp
    w = torch.zeros(z.shape[0], dtype=dtype)
    u = None
    for _ in range(n_iterations):
        u = torch.logsumexp(z - w[:, None], dim=0)
        w = torch.logsumexp(z - u[None, :], dim=1)
    return torch.exp(z - u[None, :] - w[:, None]), teacher_temp * u


def sinkhorn_cases():
    """name -> dict(logits (rows, K) f32 tensor, tt, n, f64, ref32, ref32_finite, ref32_err, log32_err, measure) of every recorded case."""
    out = {}
    for main, f64 in (("dino_sinkhorn.npz", "dino_sinkhorn.npz"), ("dino_sinkhorn_b35.npz", "dino_sinkhorn_b35_f64.npz")):
        z, z64 = _z(main), _z(f64)
        for name in sorted({k.split("/")[0] for k in z.files if "/" in k}):
            lg = z[name + "/logits"]
            out[name] = dict(logits=torch.from_numpy(lg).reshape(-1, lg.shape[-1]), shape=lg.shape, tt=float(z[name + "/teacher_temp"]),
                             n=int(z[name + "/n_iterations"]), f64=z64[name + "/f64"], ref32=z[name + "/ref32"],
                             ref32_finite=bool(z[name + "/ref32_finite"]), ref32_err=float(z[name + "/ref32_err"]),
                             log32_err=float(z[name + "/log32_err"]), measure=str(z[name + "/err_measure"]))
    return out


def test_log_domain_restatement_equals_the_reference_float64_results():
    cases = sinkhorn_cases()
    assert sorted(cases) == sorted(str(c) for c in _z("dino_sinkhorn.npz")["cases"])
    assert {c["shape"] for c in cases.values()} == {(2, 3, 1000), (2, 35, 1000)} and {c["n"] for c in cases.values()} == {1, 3}
    for name, c in cases.items():
        T, _ = sinkhorn_log_domain(c["logits"], c["tt"], c["n"])
        ref = c["f64"]
        den = ref if c["measure"] == "relative" else ref.max(axis=1, keepdims=True)
        assert float((np.abs(T.numpy() - ref) / den).max()) <= 1e-12, name
        assert np.abs(ref.sum(axis=1) - 1.0).max() <= 1e-12, name
        if c["measure"] == "relative":
            assert c["ref32_finite"] and 0 < c["ref32_err"] < 1e-5 and 0 < c["log32_err"] < 1e-5, name
            assert float(c["logits"].abs().max()) <= 1.5
        else:           # 2 * randn at tt = 0.04: exp(l / tt) overflows float32, the reference's own float32 run is not finite
            assert not c["ref32_finite"] and not np.isfinite(c["ref32"]).all(), name


def test_sinkhorn_symbols_are_declared_and_bound():
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "m3l_amd.h")).read()
    for s in SK_SYMBOLS:
        assert s + "(" in hdr and s in L.EXPORTS and hasattr(L.lib(), s), s
    assert L.lib().m3l_version() >= 404
    lib = L.lib()
    for rows, K in [(1, 4), (64, 65536), (70, 1000), (1030, 1000), (1030, 65536)]:
        splits = lib.m3l_op_sk_row_splits(rows, K)
        assert 1 <= splits <= min(rows, 64)
        assert lib.m3l_op_sk_ws_bytes(rows, K) >= splits * K * 8


def test_vtdino_carries_the_centering_keyword():
    z = _z("vtdino_step.npz")
    assert build_step_module(z).centering == "centering"
    model = build_step_module(z, centering="sinkhorn_knopp")
    assert model.centering == "sinkhorn_knopp"
    assert list(model.state_dict().keys()) == [str(k) for k in z["keys"]]
    with pytest.raises(ValueError, match="centering"):
        build_step_module(z, centering="other")


def test_dino_loss_has_the_reference_teacher_methods_and_checks_its_arguments():
    loss = m3l_amd.DINOLoss(64)
    for name in ("sinkhorn_knopp_teacher", "softmax_center_teacher", "sinkhorn_knopp_center"):
        assert callable(getattr(loss, name)), name
    t = torch.zeros(2, 3, 64)
    with pytest.raises(ValueError, match="n_iterations"):
        loss.sinkhorn_knopp_center(t, 0.04, n_iterations=0)
    with pytest.raises(ValueError, match="n_iterations"):
        loss.sinkhorn_knopp_teacher(t, 0.04, n_iterations=0)
    with pytest.raises(ValueError, match="centering"):
        loss(t, t, 0.04, centering="other")
    with pytest.raises(m3l_amd.M3LError):         # no CPU path
        loss.sinkhorn_knopp_teacher(t, 0.04)


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _gather_worker(rank, world, port, ret):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    K = 12
    pairs = torch.arange(2 * K, dtype=torch.float32).reshape(K, 2) + 100.0 * rank
    got = D._gather_col_pairs(pairs, None)
    sub = D._gather_col_pairs(pairs, dist.new_group(list(range(world))))
    assert torch.equal(got, sub)
    ret[rank] = got.numpy()
    dist.destroy_process_group()


def test_gather_col_pairs_two_ranks_gloo_in_rank_order():
    world, K = 2, 12
    port = _free_port()
    with mp.Manager() as m:
        ret = m.dict()
        mp.spawn(_gather_worker, args=(world, port, ret), nprocs=world, join=True)
        assert len(ret) == world
        want = np.stack([np.arange(2 * K, dtype=np.float32).reshape(K, 2) + 100.0 * r for r in range(world)])
        for r in range(world):
            assert ret[r].shape == (world, K, 2) and np.array_equal(ret[r], want), r
