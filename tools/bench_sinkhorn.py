"""Time of the two passes of the Sinkhorn-Knopp teacher assignment on their own (EXPERIMENTS.md "Sinkhorn-Knopp teacher").

One column pass (m3l_op_sk_colstats + m3l_op_sk_colcombine) and one row pass (m3l_op_dino_rowstats with the vector as its centre) over
cosine logits at (rows, K) = (64, 65536), the DINO shape, and (1030, 65536), an iBOT-like shape: in-library event brackets (m3l_prof_*),
mean per launch over --iters launches after --warmup, against the algorithmic bytes of each (rows * K * 4 read, 8 K or 8 rows written).
The matrices are 17 MB and 270 MB: the first stays in the 256 MB last-level cache between launches, the second does not.

Usage: python tools/bench_sinkhorn.py  (one JSON line on stdout)"""
import argparse
import ctypes as C
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import m3l_amd  # noqa: E402,F401
from m3l_amd import _lib as L  # noqa: E402
from m3l_amd import dino as D  # noqa: E402

DEV = "cuda:0"


def classes():
    lib = L.lib()
    out = {}
    for i in range(lib.m3l_prof_count()):
        name = C.create_string_buffer(96)
        ms, n, w, b = C.c_double(), C.c_long(), C.c_double(), C.c_double()
        lib.m3l_prof_get(i, name, 96, C.byref(ms), C.byref(n), C.byref(w), C.byref(b))
        if n.value:
            out[name.value.decode()] = {"us_per_launch": round(ms.value / n.value * 1e3, 1), "launches": n.value,
                                        "mb_per_launch": round(b.value / n.value / 1e6, 2), "tb_per_s": round(b.value / ms.value / 1e9, 3)}
    return out


def passes(rows, K, tt, iters, warmup):
    lib = L.lib()
    g = torch.Generator().manual_seed(rows)
    x = torch.nn.functional.normalize(torch.randn(rows, 32, generator=g), dim=-1).to(DEV)
    W = (torch.nn.functional.normalize(torch.randn(K, 32, generator=g), dim=-1) * (0.5 + torch.rand(K, 1, generator=g))).to(DEV)
    logits = (x @ W.t()).contiguous()
    st = torch.cuda.current_stream().cuda_stream
    ws = torch.empty(lib.m3l_op_sk_ws_bytes(rows, K), dtype=torch.uint8, device=DEV)
    pairs, center = torch.empty(K, 2, device=DEV), torch.empty(K, device=DEV)
    stats = None
    for i in range(warmup + iters):
        if i == warmup:
            torch.cuda.synchronize()
            lib.m3l_prof_begin(None, 1)
        L.check(lib.m3l_op_sk_colstats(L.ptr(logits), rows, K, 1.0 / tt, L.ptr(stats), L.ptr(ws), L.ptr(pairs), st), "m3l_op_sk_colstats")
        L.check(lib.m3l_op_sk_colcombine(L.ptr(pairs), 1, K, tt, L.ptr(center), st), "m3l_op_sk_colcombine")
        stats = D._row_stats(logits, rows, K, center, 1.0 / tt)
    torch.cuda.synchronize()
    lib.m3l_prof_end()
    return {"row_ranges": lib.m3l_op_sk_row_splits(rows, K), "kernels": classes()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    a = ap.parse_args()
    out = {"event_overhead_us": None}
    for rows, K in ((64, 65536), (1030, 65536)):
        out[f"{rows}x{K}"] = passes(rows, K, 0.04, a.iters, a.warmup)
        torch.cuda.empty_cache()
    out["event_overhead_us"] = round(L.lib().m3l_prof_event_overhead_us(torch.cuda.current_stream().cuda_stream, 200), 2)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
