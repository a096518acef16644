"""Anchors tests/tf_refs.py, the float64 yardstick of tests/test_tf_slices_gpu.py, and checks the inputs of every GPU case.  CPU only.

  * X (exact mode: forward AND the hand-written backward) against autograd through oracle.vtmae_oracle.transformer, 1e-12;
  * X against tests/golden/block_stack.npz, the reference's own pre-norm block, 1e-5 of each tensor's maximum;
  * every recipe with rnd = ident and the erf GELU is bit-equal to X; the restated fitted GELU stays within the error its header in
    m3l_amd/csrc/common.cuh states;
  * for every GPU case: the input regime (attention logits of std 2..4, mean largest probability 0.2..0.6, dominant keys in the first and in
    the last key tile, u of std ~2 reaching both GELU tails) and the slice-scale condition (no slice below 1e-3 of its tensor's maximum)."""
import os

import numpy as np
import pytest
import torch

import tf_cases as K
import tf_refs as T
from oracle import vtmae_oracle as O

F64 = torch.float64


def _rel(a, ref):
    return float((a - ref).abs().max()) / max(float(ref.abs().max()), 1e-300)


def _oracle(x, cot, P, depth, heads, dim_head):
    Pd = {"t." + k: v.to(F64).requires_grad_(True) for k, v in P.items()}
    xo = x.to(F64).requires_grad_(True)
    y = O.transformer(xo, Pd, "t.", depth, heads, dim_head)
    (y * cot.to(F64)).sum().backward()
    return {"y": y.detach(), "dx": xo.grad, **{k[2:]: v.grad for k, v in Pd.items()}}


@pytest.mark.parametrize("D,heads,dim_head,mlp,n,B", [(192, 3, 64, 384, 40, 2), (128, 1, 128, 256, 33, 2), (128, 4, 32, 128, 17, 3)])
def test_exact_matches_oracle_autograd(D, heads, dim_head, mlp, n, B):
    """outputs, input gradient and every parameter gradient; (128, 1, 128) has no to_out (heads 1, dim_head = D)"""
    P, x, cot = T.trained_like(D, 2, heads, dim_head, mlp, n, B, 16, seed=7)
    assert ("layers.0.0.to_out.0.weight" in P) == (not (heads == 1 and dim_head == D))
    ref = _oracle(x, cot, P, 2, heads, dim_head)
    got = T.tensors_of(T.run(x, cot, P, "", 2, heads, dim_head))
    assert set(got) == set(ref) == set(T.state_names(2, "layers.0.0.to_out.0.weight" in P)) | {"y", "dx"}
    for k in ref:
        assert _rel(got[k], ref[k]) <= 1e-12, (k, _rel(got[k], ref[k]))


@pytest.mark.parametrize("n", [48, 192])
def test_exact_reproduces_recorded_block(golden_dir, n):
    z = np.load(os.path.join(golden_dir, "block_stack.npz"))
    D, depth, heads, mlp = [int(v) for v in z["meta"]]
    P = {k[len("param/"):]: torch.tensor(z[k]) for k in z.files if k.startswith("param/")}
    res = T.run(torch.tensor(z[f"n{n}/x"]), torch.tensor(z[f"n{n}/cot"]), P, "", depth, heads, D // heads)
    assert _rel(res["layers"][0]["xout"], torch.tensor(z[f"n{n}/block0_out"]).to(F64)) <= 1e-5
    got = T.tensors_of(res)
    for k, t in got.items():
        ref = torch.tensor(z[f"n{n}/{k}" if k in ("y", "dx") else f"n{n}/grad/{k}"]).to(F64)
        assert _rel(t, ref) <= 1e-5, (k, _rel(t, ref))


@pytest.mark.parametrize("name", sorted(T._RECIPES))
@pytest.mark.parametrize("rb", [0, 1])
@pytest.mark.parametrize("kt", [32, None])
def test_recipe_without_rounding_is_bit_equal_to_exact(name, rb, kt):
    P, x, cot = T.trained_like(128, 2, 2, 64, 128, 40, 2, 16, seed=3)
    X = T.run(x, cot, P, "", 2, 2, 64)
    R = T.run(x, cot, P, "", 2, 2, 64, T.recipe(name, rb=rb, kt=kt, rnd=T.ident, fit_gelu=False))
    for k, t in T.tensors_of(X).items():
        assert torch.equal(t, T.tensors_of(R)[k]), k
    for lx, lr in zip(X["layers"], R["layers"]):
        assert sorted(lx) == sorted(("xn1", "qkv", "o", "lse", "x1", "xn2", "u", "h", "xout"))
        for k in lx:
            assert torch.equal(lx[k], lr[k]), k


def test_rounding_recipes_differ_where_the_plan_says():
    """the emulated-bf16 modes are not the exact one, the residual-bf16 mode is not the fp32-residual one, and a rounded tensor holds bf16 values"""
    P, x, cot = T.trained_like(128, 2, 2, 64, 128, 40, 2, 16, seed=3)
    X = T.run(x, cot, P, "", 2, 2, 64)
    R0 = T.run(x, cot, P, "", 2, 2, 64, T.recipe("perop"))
    R1 = T.run(x, cot, P, "", 2, 2, 64, T.recipe("perop", rb=True))
    R3 = T.run(x, cot, P, "", 2, 2, 64, T.recipe("block3"))
    assert 1e-4 < _rel(R0["y"], X["y"]) < 5e-2 and 1e-4 < _rel(R0["dx"], X["dx"]) < 1e-1
    assert not torch.equal(R0["dx"], R1["dx"]) and not torch.equal(R0["dx"], R3["dx"]) and torch.equal(R0["y"], R3["y"])
    for k in ("xn1", "qkv", "o", "xn2", "u", "h"):
        assert torch.equal(R0["layers"][1][k], T.bf16_rnd(R0["layers"][1][k])), k
    assert not torch.equal(R0["layers"][1]["x1"], T.bf16_rnd(R0["layers"][1]["x1"]))
    assert torch.equal(R1["layers"][1]["x1"], T.bf16_rnd(R1["layers"][1]["x1"])) and torch.equal(R1["dx"], T.bf16_rnd(R1["dx"]))


def test_fitted_gelu_restatement():
    """common.cuh: 'max |error| 2.5e-5 on gelu, 1.1e-4 on its derivative'; the derivative is that of the fitted function itself"""
    x = torch.linspace(-12, 12, 240001, dtype=F64)
    assert float((T.gelu_fit(x) - T.gelu_erf(x)).abs().max()) <= 2.6e-5
    assert float((T.gelu_fit_grad(x) - T.gelu_erf_grad(x)).abs().max()) <= 1.2e-4
    xi = torch.linspace(-7.9, 7.9, 1001, dtype=F64).requires_grad_(True)
    (g,) = torch.autograd.grad(T.gelu_fit(xi).sum(), xi)
    assert float((g - T.gelu_fit_grad(xi.detach())).abs().max()) <= 1e-12
    xe = torch.linspace(-6, 6, 1001, dtype=F64).requires_grad_(True)
    (ge,) = torch.autograd.grad(torch.nn.functional.gelu(xe).sum(), xe)
    assert float((ge - T.gelu_erf_grad(xe.detach())).abs().max()) <= 1e-14


def test_case_table_is_what_the_gpu_file_runs():
    ids = [c.id for c in K.CASES]
    assert len(set(ids)) == len(ids)
    fams = {c.family for c in K.CASES}
    assert fams == {"perop", "perop_dh", "block1", "block3", "mega1", "mega2", "mega3", "rowtile_tt12", "rowtile_tt6", "rowtile_auto", "rowln"}
    for fam in ("perop", "block1", "block3", "mega3", "rowtile_tt12", "rowln"):
        assert {1, 2} <= {c.depth for c in K.CASES if c.family == fam}, fam          # one depth-1 case per family
    assert [c.family for c in K.CASES if c.B * c.n > 1000] == ["rowtile_auto"]          # the one large M


@pytest.mark.parametrize("case", K.CASES, ids=lambda c: c.id)
def test_case_input_regime(case):
    P, x, cot = K.inputs_of(case)
    r = T.regime(x.to(F64), {k: v.to(F64) for k, v in P.items()}, case.heads, case.dim_head)
    print(f"\n[regime] {case.id}: {r}")
    if case.n > 1:
        assert 2.0 <= r["logit_std"] <= 4.0 and 0.2 <= r["max_prob"] <= 0.6, r
    else:
        assert r["max_prob"] == 1.0           # a softmax over one key: nothing to be peaked about
    if case.n > 32:                           # more than one key tile: dominant keys met late by some queries, early by others
        assert r["dom_last"] > 0 and r["dom_first"] > 0, r
    assert 1.7 <= r["u_std"] <= 2.3 and r["u_dip"] >= 0.05 and r["u_tail"] >= 0.05, r
    # the planted inputs: mixed-sign LayerNorm gains, outlier channels, one small sample, a cotangent that is heavier in the last row tile
    g1 = P["layers.0.0.norm.weight"]
    assert float(g1.min()) < -0.25 and float(g1.max()) > 0.25 and float(g1.abs().min()) >= 0.25 and float(g1.abs().max()) <= 3.0
    ch = x[1:].reshape(-1, case.D).std(0)
    assert int((ch > 20.0).sum()) == 3 or (case.B - 1) * case.n < 16           # (three rows do not make a standard deviation)
    assert float(x[0].abs().max()) < 0.1 * float(x[1:].abs().max())
    M, t = case.B * case.n, case.tile
    c2 = cot.reshape(M, case.D).pow(2).sum(1)
    r0 = t * ((M - 1) // t)
    if r0 > 0:
        assert float(c2[r0:].mean()) > 2.0 * float(c2[:r0].mean())


@pytest.mark.parametrize("case", K.CASES, ids=lambda c: c.id)
def test_case_slice_scale(case):
    """max|X_slice| >= 1e-3 max|X_tensor| for every slice the GPU file compares.  The one structural exception: with n = 1 the softmax is the
    constant 1, so the gradient of the q and k rows is exactly zero in exact arithmetic (and must be in the kernels: their bound is then 0)."""
    X = K.reference(case, "X")
    count = 0
    for name, x in X.items():
        top = float(x.abs().max())
        for kind, label, idx in K.slices(name, x.shape, case):
            count += 1
            m = float(K.take(x, idx).abs().max())
            if K.structural_zero(case, kind):            # (a departure from "every slice": tf_cases.structural_zero says why, and what holds instead)
                assert m <= 1e-12 * float(X["layers.0.0.to_qkv.weight"].abs().max())
                continue
            assert m >= K.SLICE_FLOOR * top, (name, label, m, top)
    assert count > 20
