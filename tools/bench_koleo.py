"""Time of the KoLeo regulariser, forward + backward (EXPERIMENTS.md "KoLeo regulariser").

At (groups, n, D) = (2, 32, 256), the DINO step's two global views at B = 32, (2, 512, 384) and (1, 4096, 384), on planted rows
(tests/koleo_cases.py):
  hip    KoLeoFn forward + backward (3 + 1 launches): mean wall time per iteration from CUDA events around --iters iterations after --warmup,
         and, in a second loop, the in-library event brackets (m3l_prof_*) per C entry point
  eager  the same arithmetic composed from torch eager operations on the same GPU, per group — the reference's KoLeoLoss.forward
         (F.normalize, mm, the diagonal fill, max, the gather, PairwiseDistance, log, mean) and its autograd backward — timed the same way
`hip_over_eager` below 1 means the kernels are faster.  Both sides' losses are printed so that a wrong result cannot pass as a fast one.

Usage: python tools/bench_koleo.py  (one JSON line on stdout)"""
import argparse
import ctypes as C
import json
import os
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import koleo_cases as KC  # noqa: E402
import m3l_amd  # noqa: E402,F401
from m3l_amd import _lib as L  # noqa: E402
from m3l_amd import dino as D  # noqa: E402

DEV = "cuda:0"
SHAPES = ((2, 32, 256), (2, 512, 384), (1, 4096, 384))


def eager_koleo(x, groups, eps=1e-8):
    pdist = torch.nn.PairwiseDistance(2, eps=1e-8)
    total = 0
    for xg in x.chunk(groups):
        y = F.normalize(xg, eps=eps, p=2, dim=-1)
        with torch.no_grad():
            dots = torch.mm(y, y.t())
            dots.view(-1)[::(y.shape[0] + 1)].fill_(-1)
            idx = torch.max(dots, dim=1)[1]
        total = total + -torch.log(pdist(y, y[idx]) + eps).mean()
    return total


def timed(fn, iters, warmup):
    for _ in range(warmup):
        out = fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        out = fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters * 1e3, out


def classes():
    lib = L.lib()
    out = {}
    for i in range(lib.m3l_prof_count()):
        name = C.create_string_buffer(96)
        ms, n, w, b = C.c_double(), C.c_long(), C.c_double(), C.c_double()
        lib.m3l_prof_get(i, name, 96, C.byref(ms), C.byref(n), C.byref(w), C.byref(b))
        if n.value:
            out[name.value.decode()] = {"us_per_call": round(ms.value / n.value * 1e3, 1), "calls": n.value,
                                        "tflops": round(w.value / ms.value / 1e9, 2)}
    return out


def shape(groups, n, Dm, iters, warmup):
    x = torch.cat([KC.planted_rows(n, Dm, s)[0] for s in range(groups)]).to(DEV).requires_grad_(True)

    def hip():
        x.grad = None
        loss = D.KoLeoFn.apply(x, groups, 1e-8, None)
        loss.backward()
        return loss

    def eager():
        x.grad = None
        loss = eager_koleo(x, groups)
        loss.backward()
        return loss
    hip_us, hip_loss = timed(hip, iters, warmup)
    eager_us, eager_loss = timed(eager, iters, warmup)
    L.lib().m3l_prof_begin(None, 1)
    for _ in range(iters):
        hip()
    torch.cuda.synchronize()
    L.lib().m3l_prof_end()
    return {"hip_us": round(hip_us, 1), "eager_us": round(eager_us, 1), "hip_over_eager": round(hip_us / eager_us, 3), "hip_loss": float(hip_loss),
            "eager_loss": float(eager_loss), "entry_points": classes()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    a = ap.parse_args()
    out = {}
    for groups, n, Dm in SHAPES:
        out[f"{groups}x{n}x{Dm}"] = shape(groups, n, Dm, a.iters, a.warmup)
        torch.cuda.empty_cache()
    out["event_overhead_us"] = round(L.lib().m3l_prof_event_overhead_us(torch.cuda.current_stream().cuda_stream, 200), 2)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
