"""CPU-only checks of the iBOT patch loss: the C ABI declarations, the public surface (iBOTPatchLoss, the two VTDINO keywords, state-dict keys), and
the float64 yardstick of the GPU tests (tests/ibot_cases.py) against the results recorded from the reference's own iBOTPatchLoss
(tests/golden/make_golden_ibot.py).  No kernel is launched here.

The recorded cases pin their inputs by a sha256 of the float32 tensors ibot_cases.inputs builds (the float64 arrays of one case are 4 to 80 MB, a
committed file holds 1 MiB); of dS and of both kinds of probabilities the fixture holds three rows of every view in full and, over all rows, the
column sums per view, the row 2-norms and the largest magnitude.  Bars: loss 1e-12 relative, dS 1e-13 and the Sinkhorn-Knopp probabilities 2e-14
of the array's largest entry (row norms and column sums: of their own largest entry)."""
import inspect
import os
from functools import lru_cache

import numpy as np
import pytest
import torch

import ibot_cases as IC
import m3l_amd
from m3l_amd import _lib as L
from test_vtdino_cpu import _z, build_step_module

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
IBOT_SYMBOLS = ["m3l_op_ibot_ws_bytes", "m3l_op_ibot_loss", "m3l_op_ibot_grad", "m3l_op_ibot_center_sum", "m3l_op_gemm_tn_acc"]
CASES = [IC.case_name(*s) for s in IC.RECORDED]


def ibot_case(name):
    """-> {key: array} of one recorded case."""
    z = _z("ibot_loss.npz")
    if not any(k.startswith(name + "/") for k in z.files):
        z = _z(f"ibot_loss_{name}.npz")
    return {k[len(name) + 1:]: z[k] for k in z.files if k.startswith(name + "/")}


@lru_cache(maxsize=None)
def restated(shape):
    """(inputs, ibot_f64 with the centre, Sinkhorn-Knopp probabilities (Q, R, K), ibot_f64 with the Sinkhorn-Knopp vector) of a shape."""
    S, T, c = IC.inputs(*shape)
    p_sk, c_sk = IC.sinkhorn_f64(T)
    return (S, T, c), IC.ibot_f64(S, T, c, IC.SHAPES[shape]), p_sk.reshape(S.shape), IC.ibot_f64(S, T, c_sk, IC.SHAPES[shape])


def _close(got, ref, bar):
    return float(np.abs(np.asarray(got) - ref).max()) <= bar * float(np.abs(ref).max())


def test_ibot_symbols_are_declared_and_bound():
    hdr = open(os.path.join(ROOT, "include", "m3l_amd.h")).read()
    for s in IBOT_SYMBOLS:
        assert s + "(" in hdr and s in L.EXPORTS and hasattr(L.lib(), s), s
    lib = L.lib()
    assert lib.m3l_version() >= 406
    assert "Q R <= 65535" in hdr                                         # the launch limit is stated
    for rows, K in [(1, 4), (5, 1000), (1600, 65536), (3100, 65536), (65535, 1000)]:
        assert lib.m3l_op_ibot_ws_bytes(rows, K) >= max(rows * 4, lib.m3l_op_sk_row_splits(rows, K) * K * 4)


def test_ibot_patch_loss_is_exported_with_the_reference_buffer():
    mod = m3l_amd.iBOTPatchLoss(patch_out_dim=64)
    assert "iBOTPatchLoss" in m3l_amd.__all__ and list(mod.state_dict()) == ["center"] and not list(mod.parameters())
    assert tuple(mod.center.shape) == (1, 1, 64) and mod.student_temp == 0.1 and mod.center_momentum == 0.9 and mod.updated is True
    assert list(inspect.signature(m3l_amd.iBOTPatchLoss.__init__).parameters)[1:] == ["patch_out_dim", "student_temp", "center_momentum", "process_group"]
    assert list(inspect.signature(mod.forward).parameters) == ["student_logits", "teacher_logits", "teacher_temp", "centering", "n_iterations"]
    assert list(inspect.signature(mod.sinkhorn_knopp_teacher).parameters) == ["teacher_output", "teacher_temp", "n_masked_patches_tensor", "n_iterations"]
    for name in ("apply_center_update", "update_center", "softmax_center_teacher"):
        assert callable(getattr(mod, name))
    assert not hasattr(mod, "forward_masked") and "forward_masked" in m3l_amd.iBOTPatchLoss.__doc__
    assert "n_masked_patches_tensor" in m3l_amd.iBOTPatchLoss.__doc__
    with pytest.raises(m3l_amd.M3LError):         # no CPU path
        mod(torch.zeros(1, 4, 64), torch.zeros(1, 4, 64), 0.05)


def test_vtdino_carries_the_two_keywords_after_koleo_weight():
    names = list(inspect.signature(m3l_amd.VTDINO.__init__).parameters)
    assert names[-3:] == ["koleo_weight", "ibot", "ibot_separate_head"]
    z = _z("vtdino_step.npz")
    model = build_step_module(z)
    assert model.ibot is False and model.ibot_separate_head is False
    assert not hasattr(model, "ibot_patch_loss") and "ibot_head" not in model.student_encoder and "ibot_head" not in model.teacher_encoder
    for kw in ({"ibot": 1}, {"ibot": "yes"}, {"ibot": None}, {"ibot": True, "ibot_separate_head": 0}, {"ibot": True, "ibot_separate_head": "no"},
               {"ibot_separate_head": True}):
        with pytest.raises(ValueError, match="ibot"):
            build_step_module(z, **kw)


def test_state_dict_keys_with_and_without_the_term():
    z = _z("vtdino_step.npz")
    base = [str(k) for k in z["keys"]]
    assert list(build_step_module(z).state_dict()) == base == list(build_step_module(z, ibot=False, ibot_separate_head=False).state_dict())
    shared = build_step_module(z, ibot=True)
    assert set(shared.state_dict()) - set(base) == {"ibot_patch_loss.center"} and set(base) <= set(shared.state_dict())
    assert tuple(shared.ibot_patch_loss.center.shape) == (1, 1, int(z["meta/K"])) and isinstance(shared.ibot_patch_loss, m3l_amd.iBOTPatchLoss)
    torch.manual_seed(3)
    sep = build_step_module(z, ibot=True, ibot_separate_head=True)
    head_keys = [k[len("student_encoder.dino_head."):] for k in base if k.startswith("student_encoder.dino_head.")]
    extra = set(sep.state_dict()) - set(base)
    assert extra == {"ibot_patch_loss.center"} | {f"{net}.ibot_head.{k}" for net in ("student_encoder", "teacher_encoder") for k in head_keys}
    assert list(sep.student_encoder.keys()) == ["backbone", "dino_head", "ibot_head"] == list(sep.teacher_encoder.keys())
    assert all(not p.requires_grad for p in sep.teacher_encoder["ibot_head"].parameters())
    assert all(p.requires_grad for p in sep.student_encoder["ibot_head"].parameters())
    # seeded initial values: the heads are drawn in the reference's order — student dino, student ibot, teacher dino, teacher ibot
    torch.manual_seed(3)
    again = build_step_module(z, ibot=True, ibot_separate_head=True)
    for k, v in sep.state_dict().items():
        assert torch.equal(v, again.state_dict()[k]), k
    torch.manual_seed(3)
    enc_dim = sep.student_encoder["backbone"].embed_dim
    m3l_amd.DinoVTT(image_size=int(z["meta/size"]), tactile_size=int(z["meta/size"]), image_patch_size=int(z["meta/patch"]),
                    tactile_patch_size=int(z["meta/patch"]), dim=int(z["meta/dim"]), depth=int(z["meta/depth"]), heads=int(z["meta/heads"]),
                    mlp_dim=int(z["meta/mlp"]), num_tactiles=2, num_register_tokens=1)
    heads = [m3l_amd.DINOHead(enc_dim, int(z["meta/K"]), hidden_dim=int(z["meta/hidden"]), bottleneck_dim=int(z["meta/bottleneck"])) for _ in range(4)]
    for head, (net, name) in zip(heads, [("student_encoder", "dino_head"), ("student_encoder", "ibot_head"), ("teacher_encoder", "dino_head"),
                                         ("teacher_encoder", "ibot_head")]):
        for k, v in head.state_dict().items():
            assert torch.equal(v, sep.state_dict()[f"{net}.{name}.{k}"]), (net, name, k)
    # the moving average and the optimiser see the new head through the two encoders
    assert len(list(sep.student_encoder.parameters())) == len(list(sep.teacher_encoder.parameters())) == len(list(shared.student_encoder.parameters())) + 8
    sep.optim_partial = lambda groups: torch.optim.SGD(groups, lr=0.1)
    opt, _, _ = sep.configure_optimizers(5, 3)
    in_opt = {id(p) for g in opt.param_groups for p in g["params"]}
    assert all(id(p) in in_opt for p in sep.student_encoder["ibot_head"].parameters())
    assert not any(id(p) in in_opt for p in sep.teacher_encoder.parameters())


def test_recorded_cases_are_the_ones_the_issue_lists():
    z = _z("ibot_loss.npz")
    assert [str(c) for c in z["cases"]] == CASES == ["q1_r5_k1000", "q2_r257_k1000", "q3_r70_k1000", "q2_r300_k4096"]
    assert float(z["student_temp"]) == IC.STUDENT_TEMP and float(z["teacher_temp"]) == IC.TEACHER_TEMP and float(z["center_momentum"]) == IC.MOMENTUM
    for shape, n in IC.RECORDED.items():
        c = ibot_case(IC.case_name(*shape))
        (S, T, cen), _, _, _ = restated(shape)
        assert c["dims"].tolist() == list(shape) + [n] and c["rows"].tolist() == IC.sample_rows(shape[1])
        assert str(c["digest"]) == IC.digest(S, T, cen), "the inputs built here are not the ones the reference ran on"
        assert np.array_equal(c["center_used"], cen.double().numpy()) and float(np.abs(c["center_used"]).max()) > 0.1
        assert float(S.abs().max()) <= 1.5 and float(T.abs().max()) <= 1.5


@pytest.mark.parametrize("shape", list(IC.RECORDED))
def test_float64_restatement_equals_the_reference_float64_results(shape):
    c = ibot_case(IC.case_name(*shape))
    _, r, p_sk, r_sk = restated(shape)
    rows = c["rows"].tolist()
    assert abs(r["loss"] - float(c["loss"])) <= 1e-12 * abs(float(c["loss"]))
    assert abs(r_sk["loss"] - float(c["loss_sk"])) <= 1e-12 * abs(float(c["loss_sk"]))
    for key, arr, bar in (("dS", r["dS"], 1e-13), ("probs", r["probs"], 1e-13), ("sk", p_sk, 2e-14)):
        s = IC.summaries(arr)
        assert float(np.abs(arr[:, rows] - c[key + "/rows"]).max()) <= bar * float(c[key + "/amax"]), key
        assert abs(float(s["amax"]) - float(c[key + "/amax"])) <= bar * float(c[key + "/amax"]), key
        assert _close(s["colsum"], c[key + "/colsum"], bar) and _close(s["rownorm"], c[key + "/rownorm"], bar), key
    assert _close(IC.summaries(r_sk["dS"])["rownorm"], c["dS_sk/rownorm"], 1e-13)
    assert _close(r["pending"], c["pending"], 1e-13) and _close(r["center_after"], c["center_after"], 1e-13)
    # every teacher row is a distribution: the identity the kernels' formula rests on
    assert float(np.abs(r["probs"].sum(-1) - 1).max()) <= 1e-12 and float(np.abs(p_sk.sum(-1) - 1).max()) <= 1e-12


def test_n_masked_patches_tensor_cancels():
    """The reference's sinkhorn_knopp_teacher was recorded on one case with n_masked_patches_tensor = 7 and = 1000: the same probabilities."""
    c = ibot_case("q3_r70_k1000")
    assert c["sk_n_masked"].tolist() == [7, 1000]
    assert float(np.abs(c["sk/rows"] - c["sk_other/rows"]).max()) <= 1e-15 * float(c["sk/amax"])
    assert all(ibot_case(n)["sk_n_masked"].shape == (1,) for n in CASES if n != "q3_r70_k1000")


@pytest.mark.parametrize("stem", ["vtdino_ibot_step", "vtdino_ibot_sk_step"])
def test_step_fixtures_hold_what_the_issue_asks(stem):
    z, zp = _z(stem + ".npz"), _z("vtdino_ibot_step.npz")
    assert int(z["meta/B"]) == 8 and int(z["meta/n_global"]) == 2 and tuple(z["meta/global_scale"]) == (0.5, 0.8)
    assert str(z["meta/centering"]) == ("centering" if stem == "vtdino_ibot_step" else "sinkhorn_knopp")
    for s in (1, 2):
        R = 8 * int(z[f"step{s}/patches_per_view_row"])
        assert R >= 288 and R > 255 and R % 64 and R % 256, R
        assert int(z[f"step{s}/patches_per_view_row"]) == 3 * zp[f"mask/{s - 1}/global/0"].shape[1]
        total, dino, ibot = (float(z[f"step{s}/{k}"]) for k in ("loss", "dino_loss", "ibot_loss"))
        assert abs(total - dino - ibot) <= 1e-12 * total and ibot > 0
        assert not np.array_equal(zp[f"mask/{s - 1}/global/0"], zp[f"mask/{s - 1}/global/1"])
    if stem == "vtdino_ibot_step":
        assert not z["step1/ibot_center_used"].any() and z["step2/ibot_center_used"].any() and z["step1/ibot_pending"].any()
        # the one-step delay: step 2 used momentum * 0 + (1 - momentum) * pending / (Q B)
        np.testing.assert_allclose(z["step2/ibot_center_used"], 0.1 * z["step1/ibot_pending"] / 16, rtol=1e-6, atol=1e-9)
