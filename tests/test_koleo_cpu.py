"""CPU-only checks of the KoLeo regulariser: the C ABI declarations, the public surface (KoLeoLoss, the VTDINO keyword), the float64 yardstick of
the GPU tests (tests/koleo_cases.py) against the results recorded from the reference's own KoLeoLoss (tests/golden/make_golden_koleo.py), and
the condition under which the GPU tests compare neighbour indices exactly, for every input they use.  No kernel is launched here."""
import os

import numpy as np
import pytest
import torch

import koleo_cases as KC
import m3l_amd
from m3l_amd import _lib as L
from test_vtdino_cpu import _z, build_step_module

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KOLEO_SYMBOLS = ["m3l_op_koleo_ws_bytes", "m3l_op_koleo_fwd", "m3l_op_koleo_bwd"]
CASES = ["single_1x192", "pair_2x192", "tie_6x192", "zero_5x64", "randn_35x256", "randn_64x192", "randn_67x100", "randn_33x50", "planted_130x256"]


def koleo_case(name):
    z = _z("dino_koleo.npz")
    return {k: z[f"{name}/{k}"] for k in ("x", "loss64", "grad64", "indices", "loss32", "grad32", "loss32_err", "grad32_err", "gap")}


def test_koleo_symbols_are_declared_and_bound():
    hdr = open(os.path.join(ROOT, "include", "m3l_amd.h")).read()
    for s in KOLEO_SYMBOLS:
        assert s + "(" in hdr and s in L.EXPORTS and hasattr(L.lib(), s), s
    lib = L.lib()
    assert lib.m3l_version() >= 405
    for groups, n, D in [(1, 1, 1), (2, 32, 256), (2, 512, 384), (1, 4096, 1024), (65535, 1, 7), (15, 4096, 50)]:
        assert lib.m3l_op_koleo_ws_bytes(groups, n, D) >= groups * n * 8


def test_koleo_loss_is_exported_and_has_no_state():
    mod = m3l_amd.KoLeoLoss()
    assert "KoLeoLoss" in m3l_amd.__all__ and len(mod.state_dict()) == 0 and not list(mod.parameters()) and not list(mod.buffers())
    assert callable(mod.pairwise_NNs_inner) and mod.last is None
    with pytest.raises(m3l_amd.M3LError):         # no CPU path
        mod(torch.zeros(4, 8))


def test_vtdino_carries_the_koleo_weight_keyword():
    z = _z("vtdino_step.npz")
    assert build_step_module(z).koleo_weight == 0.0
    model = build_step_module(z, koleo_weight=0.1)
    assert model.koleo_weight == 0.1 and isinstance(model.koleo_loss, m3l_amd.KoLeoLoss)
    assert list(model.state_dict().keys()) == [str(k) for k in z["keys"]]
    for bad in (-1, -1e-9, float("nan")):
        with pytest.raises(ValueError, match="koleo_weight"):
            build_step_module(z, koleo_weight=bad)


def test_recorded_cases_are_the_ones_the_issue_lists():
    z = _z("dino_koleo.npz")
    assert [str(c) for c in z["cases"]] == CASES
    shapes = [koleo_case(c)["x"].shape for c in CASES]
    assert shapes == [(1, 192), (2, 192), (6, 192), (5, 64), (35, 256), (64, 192), (67, 100), (33, 50), (130, 256)]
    x = koleo_case("tie_6x192")["x"]
    assert np.array_equal(x[0], x[1]) and np.array_equal(x[0], x[4]) and not np.array_equal(x[0], x[2])
    assert not koleo_case("zero_5x64")["x"][2].any()
    for (n, D), name in zip(KC.RANDOM_SHAPES, CASES[4:8]):
        assert np.array_equal(koleo_case(name)["x"], KC.random_rows(n, D, 0).numpy()), name
    assert np.array_equal(koleo_case("planted_130x256")["x"], KC.planted_rows(130, 256, 0)[0].numpy())


@pytest.mark.parametrize("name", CASES)
def test_float64_restatement_equals_the_reference_float64_results(name):
    c = koleo_case(name)
    r = KC.koleo_f64(c["x"])
    assert np.array_equal(r["indices"], c["indices"]), name
    assert abs(r["loss"] - float(c["loss64"])) <= 1e-12 * max(1.0, abs(float(c["loss64"])))
    assert float(np.abs(r["grad"] - c["grad64"]).max()) <= 1e-12 * float(np.abs(c["grad64"]).max())
    # the reference's own float32 run: the room the GPU bounds (1e-4) leave is summation order only
    assert float(c["loss32_err"]) < 1e-6 and float(c["grad32_err"]) < 1e-6


def test_lowest_index_wins_an_exact_tie_and_a_single_row_is_its_own_neighbour():
    assert koleo_case("tie_6x192")["indices"][[0, 1, 4]].tolist() == [1, 0, 0]
    assert koleo_case("zero_5x64")["indices"][2] == 0                    # every product of the zero row is 0
    assert koleo_case("single_1x192")["indices"].tolist() == [0] and not koleo_case("single_1x192")["grad64"].any()
    assert koleo_case("pair_2x192")["indices"].tolist() == [1, 0]
    # identical rows: d = sqrt(D) 1e-8 from the explicit difference, and a finite, large gradient
    r = KC.koleo_f64(koleo_case("tie_6x192")["x"])
    np.testing.assert_allclose(r["dist"][[0, 1, 4]], np.sqrt(192) * 1e-8, rtol=1e-12)
    assert np.isfinite(r["grad"]).all() and float(np.abs(r["grad"]).max()) > 1e3


@pytest.mark.parametrize("name", CASES)
def test_recorded_inputs_satisfy_the_gap_condition(name):
    c = koleo_case(name)
    gap = KC.neighbour_gap(c["x"])
    assert gap >= KC.GAP and (gap == float(c["gap"]) or abs(gap - float(c["gap"])) <= 1e-12)
    if name.startswith("randn"):
        assert 3 <= KC.in_degree(c["indices"]).max() <= 4


@pytest.mark.parametrize("name", sorted(KC.GPU_INPUTS))
def test_gpu_test_inputs_satisfy_the_gap_condition(name):
    kind, n, D, seeds = KC.GPU_INPUTS[name]
    assert kind == "randn" or D != 50              # the planted construction's gap falls to 1e-5 there
    for seed, x in zip(seeds, KC.gpu_input(name)):
        assert x.shape == (n, D) and x.dtype == torch.float32
        assert KC.neighbour_gap(x.numpy()) >= KC.GAP
        if kind == "planted":
            rows, what = KC.planted_rows(n, D, seed)
            deg, what = KC.in_degree(KC.koleo_f64(rows.numpy())["indices"]), what.numpy()
            dropped = 3 * -(-n // 3) - n                                 # far children left out: their anchors have in-degree 1
            assert np.bincount(deg[what == 0], minlength=3).tolist() == [0, dropped, (what == 0).sum() - dropped]
            assert (deg[what == 1] == 1).all() and (deg[what == 2] == 0).all()
            assert abs(float((deg == 0).mean()) - 1 / 3) < 0.02


def test_step_fixture_margins_hold_for_every_step_and_view():
    z = _z("vtdino_koleo_step.npz")
    assert int(z["meta/steps"]) == 2 and float(z["meta/koleo_weight"]) == 0.1 and int(z["meta/n_global"]) == 2 and int(z["meta/B"]) == 6
    for s in (1, 2):
        gap, diff = z[f"margin/step{s}/gap"], z[f"margin/step{s}/bf16_product_diff"]
        assert gap.shape == (2,) and (gap >= KC.GAP).all() and (gap >= 10 * diff).all(), (s, gap, diff)
        assert z[f"step{s}/koleo_indices"].shape == (2, 6)
        assert abs(float(z[f"step{s}/loss"]) - float(z[f"step{s}/dino_loss"]) - float(z[f"step{s}/koleo_loss"])) <= 1e-12 * float(z[f"step{s}/loss"])
        assert not np.array_equal(z[f"mask/{s - 1}/global/0"], z[f"mask/{s - 1}/global/1"])
