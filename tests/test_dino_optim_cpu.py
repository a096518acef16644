"""CPU checks of the DINO optimizer stack (m3l_amd/optim.py, m3l_dino_opt_step): the schedulers against the values recorded from the
reference's own classes (tests/golden/make_golden_dino_opt.py), the new symbol and its argument checks (all made before any device call, so
they run without a GPU), the segment-table builder, and what DinoAdamW does on the host: layout, gradient views, idle tracking, groups."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import m3l_amd
from m3l_amd import _lib as L
from m3l_amd.optim import build_segments

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")


def _two_groups(opt_cls, wd, **kw):
    a, b = torch.nn.Parameter(torch.zeros(2, 2)), torch.nn.Parameter(torch.zeros(2))
    return opt_cls([{"params": [a]}, {"params": [b], "WD_exclude": True, "weight_decay": 0.0}], lr=5e-4, weight_decay=wd, **kw), (a, b)


# ------------------------------------------------------------------------------------------------------------------------ schedulers
@pytest.mark.parametrize("case", ["wd_up", "wd_down"])
def test_schedulers_equal_the_reference_record(case):
    """lr and wd of both groups after construction and after each of 16 scheduler steps (one past T_max), to 1e-15 relative: the same
    double arithmetic as the reference's classes."""
    z = np.load(os.path.join(GOLDEN, "dino_opt_schedules.npz"), allow_pickle=False)
    m = {k[len("meta/"):]: z[k] for k in z.files if k.startswith("meta/")}
    w0, w1 = float(m[case + "/ref_weight_decay"]), float(m[case + "/final_weight_decay"])
    assert float(m["base_lr"]) == 5e-4
    opt, (a, b) = _two_groups(torch.optim.AdamW, w0)
    lr_s = m3l_amd.WarmupCosineScheduler(opt, steps_per_epoch=int(m["steps_per_epoch"]), start_lr=float(m["start_lr"]), T_max=int(m["T_max"]),
                                         warmup_epochs=int(m["warmup_epochs"]), final_lr=float(m["final_lr"]))
    wd_s = m3l_amd.CosineWDSchedule(opt, ref_weight_decay=w0, final_weight_decay=w1, T_max=int(m["T_max"]))
    lr, wd, ret = [[g["lr"] for g in opt.param_groups]], [[g["weight_decay"] for g in opt.param_groups]], []
    steps = int(m["steps"])
    assert steps == int(m["T_max"]) + 1
    for _ in range(steps):
        a.grad, b.grad = torch.zeros_like(a), torch.zeros_like(b)
        opt.step()
        lr_s.step()
        ret.append(wd_s.step())
        lr.append([g["lr"] for g in opt.param_groups])
        wd.append([g["weight_decay"] for g in opt.param_groups])
    np.testing.assert_allclose(np.array(lr), z[case + "/lr"], rtol=1e-15, atol=0)
    np.testing.assert_allclose(np.array(wd), z[case + "/wd"], rtol=1e-15, atol=0)
    np.testing.assert_allclose(np.array(ret), z[case + "/wd_returned"], rtol=1e-15, atol=0)
    assert all(w[1] == 0.0 for w in wd), "the WD_exclude group was given a weight decay"
    assert opt.param_groups[0]["initial_lr"] == 5e-4


def test_schedulers_accept_and_drive_dino_adamw():
    """LRScheduler refuses anything that is not a torch.optim.Optimizer; DinoAdamW is one, and both schedulers write its groups."""
    opt, _ = _two_groups(m3l_amd.DinoAdamW, 0.05, max_grad_norm=10.0)
    assert isinstance(opt, torch.optim.Optimizer)
    lr_s = m3l_amd.WarmupCosineScheduler(opt, steps_per_epoch=5, start_lr=1e-5, T_max=15, warmup_epochs=1, final_lr=1e-6)
    wd_s = m3l_amd.CosineWDSchedule(opt, ref_weight_decay=0.05, final_weight_decay=0.4, T_max=15)
    assert opt.param_groups[0]["lr"] == opt.param_groups[1]["lr"] == 1e-5 + 0.2 * (5e-4 - 1e-5)
    assert isinstance(lr_s, torch.optim.lr_scheduler.LRScheduler)
    w = wd_s.step()
    assert opt.param_groups[0]["weight_decay"] == w > 0.05 and opt.param_groups[1]["weight_decay"] == 0.0
    assert opt.param_groups[1]["WD_exclude"] is True and opt.param_groups[0]["initial_lr"] == 5e-4


# --------------------------------------------------------------------------------------------------------------------------- symbols
def test_new_symbol_is_declared_bound_and_versioned():
    hdr = open(os.path.join(ROOT, "include", "m3l_amd.h")).read()
    declared = set(re.findall(r"\b(m3l_[a-z0-9_]+)\s*\(", hdr))
    assert "m3l_dino_opt_step" in declared
    assert "m3l_dino_opt_step" in L.EXPORTS
    assert hasattr(L.lib(), "m3l_dino_opt_step")
    assert L.lib().m3l_version() >= 407
    for name in ("DinoAdamW", "WarmupCosineScheduler", "CosineWDSchedule"):
        assert name in m3l_amd.__all__ and hasattr(m3l_amd, name)


def _call(**over):
    """m3l_dino_opt_step on made-up addresses: only calls that the argument checks refuse (before any device call) may be made here."""
    lr, wd = (C.c_float * 9)(*([1e-3] * 9)), (C.c_float * 9)(*([0.01] * 9))
    a = dict(params=0x10000, grads=0x20000, exp_avg=0x30000, exp_avg_sq=0x40000, teacher=None, n=100, seg_start=0x50000, seg_group=0x60000,
             n_segments=1, lr=lr, wd=wd, n_groups=2, step=1, max_grad_norm=0.0, norm_ws=None)
    a.update(over)
    return L.lib().m3l_dino_opt_step(a["params"], a["grads"], a["exp_avg"], a["exp_avg_sq"], a["teacher"], a["n"], a["seg_start"], a["seg_group"],
                                     a["n_segments"], a["lr"], a["wd"], a["n_groups"], 0.9, 0.999, 1e-8, a["step"], 1.0, a["max_grad_norm"],
                                     a["norm_ws"], 1, 0.99, None)


@pytest.mark.parametrize("over,word", [
    (dict(n_segments=0), "segments"), (dict(n_groups=9), "groups"), (dict(n_groups=0), "groups"), (dict(n=0), "n=0"), (dict(step=0), "step=0"),
    (dict(params=0x10004), "aligned"), (dict(grads=0x20008), "aligned"), (dict(exp_avg=0x30004), "aligned"), (dict(exp_avg_sq=0x4000c), "aligned"),
    (dict(teacher=0x70004), "aligned"), (dict(params=None), "null"), (dict(seg_start=None), "null"), (dict(seg_group=None), "null"),
    (dict(max_grad_norm=1.0), "workspace")])
def test_invalid_arguments_return_an_error_code(over, word):
    assert _call(**over) != 0
    assert word in L.last_error(), L.last_error()


# -------------------------------------------------------------------------------------------------------------------- segment builder
def test_build_segments_merges_neighbours_of_one_group():
    assert build_segments([(0, 4, 0), (4, 9, 0), (9, 10, 1), (10, 30, 1)], 30) == ([0, 9, 30], [0, 1])
    assert build_segments([(0, 5, 0)], 5) == ([0, 5], [0])


def test_build_segments_splits_around_idle_parameters():
    # idle first, between two of one group, and last
    assert build_segments([(0, 3, -1), (3, 7, 0), (7, 8, -1), (8, 20, 0), (20, 21, 1), (21, 25, -1)], 25) == ([0, 3, 7, 8, 20, 21, 25], [-1, 0, -1, 0, 1, -1])
    # neighbouring idle parameters of different groups merge into one idle segment
    assert build_segments([(0, 3, 0), (3, 5, -1), (5, 9, -1), (9, 12, 1)], 12) == ([0, 3, 9, 12], [0, -1, 1])
    # everything idle
    assert build_segments([(0, 3, -1), (3, 5, -1)], 5) == ([0, 5], [-1])


def test_build_segments_orders_spans_and_fills_gaps():
    # any order in; a stretch nobody owns (a parameter of the flat buffer that is not the optimizer's) is idle
    assert build_segments([(10, 12, 1), (0, 4, 0)], 16) == ([0, 4, 10, 12, 16], [0, -1, 1, -1])
    for bad in ([(0, 4, 0), (3, 6, 0)], [(0, 4, 0), (4, 9, 1)]):
        with pytest.raises(ValueError):
            build_segments(bad, 8)
    with pytest.raises(ValueError):
        build_segments([], 0)


def test_build_segments_invariants_on_random_layouts():
    g = torch.Generator().manual_seed(0)
    for _ in range(50):
        lens = torch.randint(1, 9, (int(torch.randint(1, 30, (1,), generator=g)),), generator=g).tolist()
        groups = torch.randint(-1, 3, (len(lens),), generator=g).tolist()
        spans, at = [], 0
        for ln, k in zip(lens, groups):
            spans.append((at, at + ln, k))
            at += ln
        starts, segs = build_segments(spans, at)
        assert starts[0] == 0 and starts[-1] == at and len(starts) == len(segs) + 1
        assert all(a < b for a, b in zip(starts, starts[1:])) and all(x != y for x, y in zip(segs, segs[1:]))
        per_elem = [k for ln, k in zip(lens, groups) for _ in range(ln)]
        assert per_elem == [k for (a, b), k in zip(zip(starts, starts[1:]), segs) for _ in range(b - a)]


# ------------------------------------------------------------------------------------------------------------- the optimizer's host side
def _toy():
    torch.manual_seed(0)
    net = torch.nn.ModuleDict({"a": torch.nn.Linear(3, 5), "unused": torch.nn.Linear(2, 2), "b": torch.nn.Linear(5, 1)})
    params = list(net.parameters())
    groups = [{"params": [p for p in params if p.dim() >= 2]}, {"params": [p for p in params if p.dim() < 2], "WD_exclude": True, "weight_decay": 0.0}]
    return net, groups


def test_flat_layout_gradient_views_and_idle_tracking():
    net, groups = _toy()
    before = {k: v.detach().clone() for k, v in net.state_dict().items()}
    opt = m3l_amd.DinoAdamW(groups, lr=5e-4, weight_decay=0.05)
    assert all(torch.equal(v, before[k]) for k, v in net.state_dict().items()) and list(net.state_dict()) == list(before)
    n = sum(p.numel() for p in net.parameters())
    assert opt.flat.numel() == opt.flat_params.numel() == opt.exp_avg.numel() == n == 15 + 4 + 5 + 5 + 2 + 1
    # group-major: the three matrices, then the three vectors
    off = 0
    for g in opt.param_groups:
        for p in g["params"]:
            assert p.data_ptr() == opt.flat_params.data_ptr() + 4 * off and p.grad.data_ptr() == opt.flat.data_ptr() + 4 * off
            off += p.numel()
    assert build_segments(opt.segment_spans(frozenset(id(p) for p in net.parameters())), n) == ([0, 24, n], [0, 1])
    views = [p.grad for p in net.parameters()]
    net["b"](net["a"](torch.ones(2, 3))).sum().backward()
    assert all(p.grad is v for p, v in zip(net.parameters(), views)), "the backward replaced a gradient view"
    assert float(opt.flat.abs().sum()) > 0
    active = opt._active()
    assert active == frozenset(id(p) for name in ("a", "b") for p in net[name].parameters())
    # unused.weight sits between a.weight and b.weight in group 0, unused.bias between the two biases of group 1
    assert build_segments(opt.segment_spans(active), n) == ([0, 15, 19, 24, 29, 31, n], [0, -1, 0, 1, -1, 1])
    opt.zero_grad()                       # torch's default set_to_none=True must not cut the views loose
    assert all(p.grad is v for p, v in zip(net.parameters(), views)) and float(opt.flat.abs().sum()) == 0.0
    assert opt._active() == frozenset()
    opt.zero_grad(set_to_none=True)
    assert all(p.grad is v for p, v in zip(net.parameters(), views))


def test_construction_errors_and_cpu_step_is_refused():
    net, groups = _toy()
    with pytest.raises(ValueError):
        m3l_amd.DinoAdamW([{"params": [p]} for p in net.parameters()] + [{"params": [torch.nn.Parameter(torch.zeros(1))]} for _ in range(3)], lr=1e-3)
    with pytest.raises(ValueError):
        m3l_amd.DinoAdamW([{"params": groups[0]["params"]}, {"params": groups[1]["params"], "eps": 1e-6}], lr=1e-3)
    opt = m3l_amd.DinoAdamW(groups, lr=1e-3)
    with pytest.raises(L.M3LError):        # no eager fallback: the update is a HIP kernel
        opt.step()


def test_state_dict_round_trip_on_the_host():
    net, groups = _toy()
    opt = m3l_amd.DinoAdamW(groups, lr=5e-4, weight_decay=0.05)
    opt.step_count = 7
    opt.exp_avg.copy_(torch.arange(opt.flat.numel(), dtype=torch.float32))
    opt.exp_avg_sq.copy_(torch.arange(opt.flat.numel(), dtype=torch.float32) * 0.5)
    opt.param_groups[0]["lr"], opt.param_groups[0]["weight_decay"] = 1.25e-4, 0.3
    sd = opt.state_dict()
    assert sd["param_groups"][1]["WD_exclude"] is True and sd["param_groups"][0]["lr"] == 1.25e-4
    assert sd["state"][0]["exp_avg"].shape == groups[0]["params"][0].shape
    net2, groups2 = _toy()
    opt2 = m3l_amd.DinoAdamW(groups2, lr=1.0, weight_decay=0.0)
    opt2.load_state_dict(sd)
    assert opt2.step_count == 7 and torch.equal(opt2.exp_avg, opt.exp_avg) and torch.equal(opt2.exp_avg_sq, opt.exp_avg_sq)
    assert opt2.param_groups[0]["lr"] == 1.25e-4 and opt2.param_groups[0]["weight_decay"] == 0.3 and opt2.param_groups[1]["weight_decay"] == 0.0
    assert opt2.param_groups[1]["WD_exclude"] is True
