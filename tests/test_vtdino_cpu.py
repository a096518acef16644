"""CPU-only checks of the DINO self-distillation stack (m3l_amd.VTDINO, DINOHead, DINOLoss): state-dict keys and shapes, seeded initial
values, the block-mask sampler and the schedules against values recorded from the reference's own classes
(tests/golden/make_golden_vtdino.py), and the C ABI declarations.  No kernel is launched here."""
import os
import re
from functools import partial

import numpy as np
import pytest
import torch

import m3l_amd
from m3l_amd import _lib as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")

NEW_SYMBOLS = ["m3l_op_l2norm_fwd", "m3l_op_l2norm_bwd", "m3l_op_weightnorm_fwd", "m3l_op_weightnorm_bwd", "m3l_op_dino_ws_bytes",
               "m3l_op_dino_rowstats", "m3l_op_dino_loss", "m3l_op_dino_grad", "m3l_op_dino_center_sum", "m3l_op_dino_center_apply", "m3l_op_ema"]


def _z(name):
    return np.load(os.path.join(GOLDEN, name), allow_pickle=False)


def build_step_module(z, compute_dtype="fp32", **over):
    m = {k[len("meta/"):]: z[k] for k in z.files if k.startswith("meta/")}
    enc = m3l_amd.DinoVTT(image_size=int(m["size"]), tactile_size=int(m["size"]), image_patch_size=int(m["patch"]),
                          tactile_patch_size=int(m["patch"]), dim=int(m["dim"]), depth=int(m["depth"]), heads=int(m["heads"]),
                          mlp_dim=int(m["mlp"]), num_tactiles=2, num_register_tokens=1, compute_dtype=compute_dtype)
    kw = dict(encoder=enc, dino_head=partial(m3l_amd.DINOHead, out_dim=int(m["K"]), hidden_dim=int(m["hidden"]), bottleneck_dim=int(m["bottleneck"])),
              optim_cfg=None, lr_scheduler_cfg=None, wd_scheduler_cfg=None, local_mask_scale=tuple(float(v) for v in m["local_scale"]),
              global_mask_scale=tuple(float(v) for v in m["global_scale"]), num_global_masks=int(m["n_global"]), num_local_masks=int(m["n_local"]),
              min_keep_num_sensors=int(m["min_keep"]), allow_mask_overlap=False, moving_average_decay=float(m["decay"]),
              teacher_temp=float(m["teacher_temp"]))
    kw.update(over)
    model = m3l_amd.VTDINO(**kw)
    model.current_teacher_temp = float(m["teacher_temp"])
    return model


def load_step_params(model, z):
    """The fixture's initial values: student, teacher head, centre; the teacher backbone starts as the student's."""
    sd = {k[len("param/"):]: torch.from_numpy(z[k]) for k in z.files if k.startswith("param/")}
    for k in list(sd):
        if k.startswith("student_encoder.backbone."):
            sd["teacher_encoder.backbone." + k[len("student_encoder.backbone."):]] = sd[k].clone()
    model.load_state_dict(sd, strict=True)


def test_new_symbols_are_declared_bound_and_versioned():
    hdr = open(os.path.join(ROOT, "include", "m3l_amd.h")).read()
    declared = set(re.findall(r"\b(m3l_[a-z0-9_]+)\s*\(", hdr))
    for s in NEW_SYMBOLS:
        assert s in declared, f"{s} is not declared in include/m3l_amd.h"
        assert s in L.EXPORTS, f"{s} has no prototype in m3l_amd/_lib.py"
        assert hasattr(L.lib(), s)
    assert L.lib().m3l_version() >= 403
    assert L.lib().m3l_op_dino_ws_bytes(384, 65536) > 0


def test_head_state_dict_and_seeded_init_equal_the_reference():
    z = _z("dino_head_init.npz")
    in_dim, out_dim, hidden, bott = [int(v) for v in z["cfg"]]
    torch.manual_seed(5)
    head = m3l_amd.DINOHead(in_dim, out_dim, hidden_dim=hidden, bottleneck_dim=bott)
    want = {k[len("init3/"):]: z[k] for k in z.files if k.startswith("init3/")}
    sd = head.state_dict()
    assert list(sd.keys()) == list(want.keys())
    assert set(sd) == {"mlp.0.weight", "mlp.0.bias", "mlp.2.weight", "mlp.2.bias", "mlp.4.weight", "mlp.4.bias", "last_layer.weight_g",
                       "last_layer.weight_v"}
    for k, v in want.items():
        assert tuple(sd[k].shape) == v.shape, k
        assert np.array_equal(sd[k].numpy(), v), k
    assert tuple(sd["last_layer.weight_g"].shape) == (out_dim, 1) and tuple(sd["last_layer.weight_v"].shape) == (out_dim, bott)
    assert [n for n, _ in head.named_parameters()][-2:] == ["last_layer.weight_g", "last_layer.weight_v"]
    # one layer, no bias
    torch.manual_seed(6)
    head1 = m3l_amd.DINOHead(in_dim, out_dim, nlayers=1, hidden_dim=hidden, bottleneck_dim=bott, mlp_bias=False)
    want1 = {k[len("init1/"):]: z[k] for k in z.files if k.startswith("init1/")}
    assert list(head1.state_dict().keys()) == list(want1.keys()) == ["mlp.weight", "last_layer.weight_g", "last_layer.weight_v"]
    for k, v in want1.items():
        assert np.array_equal(head1.state_dict()[k].numpy(), v), k
    # a reference state dict loads strictly
    head.load_state_dict({k[len("param/"):]: torch.from_numpy(z[k]) for k in z.files if k.startswith("param/")}, strict=True)


def test_head_refuses_batchnorm():
    with pytest.raises(NotImplementedError, match="use_bn"):
        m3l_amd.DINOHead(64, 128, use_bn=True)


def test_module_state_dict_keys_and_shapes_equal_the_reference():
    z = _z("vtdino_step.npz")
    model = build_step_module(z)
    sd = model.state_dict()
    assert list(sd.keys()) == [str(k) for k in z["keys"]]
    for k, shape in zip(z["keys"], z["shapes"]):
        assert ",".join(str(d) for d in sd[str(k)].shape) == str(shape), k
    assert tuple(model.dino_loss.center.shape) == (1, int(z["meta/K"]))
    assert isinstance(model.student_encoder, torch.nn.ModuleDict) and list(model.student_encoder.keys()) == ["backbone", "dino_head"]
    assert list(model.teacher_encoder.keys()) == ["backbone", "dino_head"]
    assert all(not p.requires_grad for p in model.teacher_encoder.parameters())
    assert all(p.requires_grad for p in model.student_encoder.parameters())
    load_step_params(model, z)              # strict
    # the teacher backbone is a copy of the encoder, the teacher head is a fresh one
    fresh = build_step_module(z)
    for (n, a), (_, b) in zip(fresh.student_encoder["backbone"].named_parameters(), fresh.teacher_encoder["backbone"].named_parameters()):
        assert torch.equal(a, b) and a.data_ptr() != b.data_ptr(), n
    assert not torch.equal(fresh.student_encoder["dino_head"].mlp[0].weight, fresh.teacher_encoder["dino_head"].mlp[0].weight)


def _mask_module(cfg, scales):
    size, patch, B, n_global, n_local, overlap, min_keep = [int(v) for v in cfg]
    enc = m3l_amd.DinoVTT(image_size=size, tactile_size=32, image_patch_size=patch, tactile_patch_size=8, dim=64, depth=1, heads=1, mlp_dim=64,
                          num_tactiles=2, num_register_tokens=1)
    model = m3l_amd.VTDINO(encoder=enc, dino_head=partial(m3l_amd.DINOHead, out_dim=64, hidden_dim=32, bottleneck_dim=16), optim_cfg=None,
                           lr_scheduler_cfg=None, wd_scheduler_cfg=None, global_mask_scale=(float(scales[0]), float(scales[1])),
                           local_mask_scale=(float(scales[2]), float(scales[3])), num_global_masks=n_global, num_local_masks=n_local,
                           min_keep_num_sensors=min_keep, allow_mask_overlap=bool(overlap), teacher_temp=0.05)
    return model, torch.zeros(B, 3, size, size)


@pytest.mark.parametrize("case", ["grid8", "grid4"])
def test_sample_masks_bit_equal_to_the_reference(case):
    z = _z("vtdino_masks.npz")
    model, x = _mask_module(z[case + "/cfg"], z[case + "/scales"])
    n_global, n_local = int(z[case + "/cfg"][3]), int(z[case + "/cfg"][4])
    assert len(z[case + "/seeds"]) >= 6
    for seed in z[case + "/seeds"]:
        model.generator.manual_seed(int(seed))
        gm, lm = model.sample_masks(x)
        assert len(gm) == n_global and len(lm) == n_local
        for kind, got in (("global", gm), ("local", lm)):
            for i, m in enumerate(got):
                want = z[f"{case}/seed{int(seed)}/{kind}/{i}"]
                assert m.dtype == torch.int64 and tuple(m.shape) == want.shape, (case, seed, kind, i)
                assert np.array_equal(m.numpy(), want), (case, seed, kind, i)


@pytest.mark.parametrize("size", [64, (64, 32)])
def test_unconstrained_fast_path_equals_the_block_by_block_sampler(size):
    """With overlap allowed sample_masks draws each sample's placements in bulk; the block-by-block loop (pinned to the reference by the
    4x4 fixture above) must give the same indices from the same seed, on a square grid and on one whose two placement ranges differ."""
    enc = m3l_amd.DinoVTT(image_size=size, tactile_size=32, image_patch_size=8, tactile_patch_size=8, dim=64, depth=1, heads=1, mlp_dim=64,
                          num_tactiles=2, num_register_tokens=1)
    model = m3l_amd.VTDINO(encoder=enc, dino_head=partial(m3l_amd.DINOHead, out_dim=64, hidden_dim=32, bottleneck_dim=16), optim_cfg=None,
                           lr_scheduler_cfg=None, wd_scheduler_cfg=None, global_mask_scale=(0.48, 1.0), local_mask_scale=(0.3, 0.48),
                           num_global_masks=2, num_local_masks=3, allow_mask_overlap=True, teacher_temp=0.05)
    H, W = (size, size) if isinstance(size, int) else size
    x = torch.zeros(5, 3, H, W)
    for seed in range(4):
        model.generator.manual_seed(seed)
        gm, lm = model.sample_masks(x)
        model.generator.manual_seed(seed)
        local_size = model._sample_block_size(H // 8, W // 8, model.local_mask_scale)
        global_size = model._sample_block_size(H // 8, W // 8, model.global_mask_scale)
        for b in range(5):
            for i in range(3):
                assert torch.equal(lm[i][b], model._sample_block_mask(H // 8, W // 8, local_size)[0]), (seed, b, i)
            for i in range(2):
                assert torch.equal(gm[i][b], model._sample_block_mask(H // 8, W // 8, global_size)[0]), (seed, b, i)


def test_step_fixture_masks_reproduced_from_the_step_counter():
    z = _z("vtdino_step.npz")
    model = build_step_module(z)
    x = torch.from_numpy(z["input/image"])
    for s in range(2):
        model.generator.manual_seed(s)
        gm, lm = model.sample_masks(x)
        for i, m in enumerate(gm):
            assert np.array_equal(m.numpy(), z[f"mask/{s}/global/{i}"])
        for i, m in enumerate(lm):
            assert np.array_equal(m.numpy(), z[f"mask/{s}/local/{i}"])


def test_block_that_can_never_pass_raises_instead_of_hanging():
    model, x = _mask_module([64, 8, 2, 2, 8, 1, 4], [0.48, 1.0, 0.1, 0.1])       # int(64 * 0.1) = 6 patches -> a 2x2 block, never > 4
    model.generator.manual_seed(0)
    with pytest.raises(ValueError, match="min_keep_num_sensors"):
        model.sample_masks(x)


def test_schedules_equal_the_reference_generators():
    z = _z("vtdino_step.npz")
    iters, epochs, warm = [int(v) for v in z["sched/args"]]
    model = build_step_module(z, optim_cfg=lambda groups: torch.optim.SGD(groups, lr=0.1), lr_scheduler_cfg=lambda **kw: None,
                              moving_average_decay=[0.99, 1.0], teacher_temp=[0.04, 0.07], teacher_warmup_epochs=warm)
    opt, lr_entry, wd_entry = model.configure_optimizers(iters, epochs)
    assert wd_entry is None and lr_entry["interval"] == "step"
    assert [len(g["params"]) for g in opt.param_groups] == [int(v) for v in z["sched/group_sizes"]]
    assert all(p.dim() >= 2 for p in opt.param_groups[0]["params"]) and all(p.dim() < 2 for p in opt.param_groups[1]["params"])
    assert opt.param_groups[1]["weight_decay"] == 0.0 and opt.param_groups[1]["WD_exclude"] is True
    assert model.current_teacher_temp == 0.04
    assert np.array_equal(np.array(list(model.teacher_temp_scheduler)), z["sched/teacher_temp"])
    assert np.array_equal(np.array(list(model.momentum_scheduler)), z["sched/momentum"])
    # a tuple is accepted where the reference asserts, and a float stays a float
    assert build_step_module(z, teacher_temp=(0.04, 0.07)).teacher_temp == (0.04, 0.07)
    assert build_step_module(z).moving_average_decay == float(z["meta/decay"])


def test_online_probes_are_refused():
    z = _z("vtdino_step.npz")
    with pytest.raises(NotImplementedError, match="online probes"):
        build_step_module(z, online_probes=[torch.nn.Linear(4, 4)], online_probes_lrs=[0.1])
