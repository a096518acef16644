#!/usr/bin/env python3
"""Recorded schedules of the DINO optimizer (runs ONLY where the reference checkout is mounted; no test reads the reference).

Loads the REFERENCE's own `tactile_ssl/model/custom_scheduler.py` by path (it imports only math and torch), drives its
`WarmupCosineScheduler` and `CosineWDSchedule` over a two-group torch.optim.AdamW — group 0 decayed, group 1 `WD_exclude` with
weight_decay 0, the groups of VTDINO.configure_optimizers — in the order of the reference trainer's loop body (optimizer.step(),
lr scheduler, wd scheduler) and writes data only:

  dino_opt_schedules.npz   `meta/*` the case; per wd case `<name>/lr` and `<name>/wd`, float64 (steps + 1, 2): row 0 what the groups hold
                           after the schedulers' construction, row i what they hold after the i-th pair of scheduler steps; `<name>/wd_returned`
                           (steps,) what CosineWDSchedule.step() returned.

Case: steps_per_epoch 5, T_max 15, warmup_epochs 1, start_lr 1e-5, final_lr 1e-6, base lr 5e-4; weight decay 0.05 -> 0.4 ("wd_up") and
0.4 -> 0.05 ("wd_down"); 16 steps, one past T_max.

Usage:  python tests/golden/make_golden_dino_opt.py
"""
import importlib.util
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_golden import REF  # noqa: E402

CASE = dict(steps_per_epoch=5, T_max=15, warmup_epochs=1, start_lr=1e-5, final_lr=1e-6, base_lr=5e-4, steps=16)
WD_CASES = {"wd_up": (0.05, 0.4), "wd_down": (0.4, 0.05)}


def load_schedulers():
    spec = importlib.util.spec_from_file_location("ref_custom_scheduler", os.path.join(REF, "tactile_ssl", "model", "custom_scheduler.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m.WarmupCosineScheduler, m.CosineWDSchedule


def record(Warmup, CosineWD, ref_wd, final_wd):
    a, b = torch.nn.Parameter(torch.zeros(2, 2)), torch.nn.Parameter(torch.zeros(2))
    opt = torch.optim.AdamW([{"params": [a]}, {"params": [b], "WD_exclude": True, "weight_decay": 0.0}], lr=CASE["base_lr"], weight_decay=ref_wd)
    lr_s = Warmup(opt, steps_per_epoch=CASE["steps_per_epoch"], start_lr=CASE["start_lr"], T_max=CASE["T_max"],
                  warmup_epochs=CASE["warmup_epochs"], final_lr=CASE["final_lr"])
    wd_s = CosineWD(opt, ref_weight_decay=ref_wd, final_weight_decay=final_wd, T_max=CASE["T_max"])
    lr, wd, ret = [[g["lr"] for g in opt.param_groups]], [[g["weight_decay"] for g in opt.param_groups]], []
    for _ in range(CASE["steps"]):
        a.grad, b.grad = torch.zeros_like(a), torch.zeros_like(b)
        opt.step()
        lr_s.step()
        ret.append(wd_s.step())
        lr.append([g["lr"] for g in opt.param_groups])
        wd.append([g["weight_decay"] for g in opt.param_groups])
    return np.array(lr, dtype=np.float64), np.array(wd, dtype=np.float64), np.array(ret, dtype=np.float64)


if __name__ == "__main__":
    Warmup, CosineWD = load_schedulers()
    out = {"meta/" + k: np.asarray(v) for k, v in CASE.items()}
    out["cases"] = np.array(list(WD_CASES))
    for name, (w0, w1) in WD_CASES.items():
        out[f"meta/{name}/ref_weight_decay"], out[f"meta/{name}/final_weight_decay"] = np.float64(w0), np.float64(w1)
        out[name + "/lr"], out[name + "/wd"], out[name + "/wd_returned"] = record(Warmup, CosineWD, w0, w1)
        print(name, "lr", out[name + "/lr"][:, 0], "wd", out[name + "/wd"][:, 0], sep="\n")
    path = os.path.join(HERE, "dino_opt_schedules.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path))
