"""A/B of transformer dropout at the cfg-2 bench workload (B = 256, bf16, zero_grad + mask + fwd + bwd + Adam, one GPU):

  (a) default kernel selection, p = 0       (b) default selection, p = 0.1 (what a user pays: the encoder leaves the fused kernels)
  (c) per-op chain forced, p = 0            (d) per-op chain forced, p = 0.1 ((d) - (c) = the dropout arithmetic itself)

The per-op chain is forced with the existing switches m3l_set_attn_block(0), m3l_set_enc_mega(0), m3l_set_t192(0).  One model, the arms
interleaved over `--rounds` rounds; prints one JSON line with the median step time of every arm.
usage: python tools/dropout_ab.py [--steps 20] [--warmup 5] [--rounds 3]"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from bench import CFG2, build_model, synthetic_batch  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--batch", type=int, default=256)
    args = ap.parse_args()
    from m3l_amd import _lib as L
    from m3l_amd.parallel import FlatAdam, GradSync
    lib = L.lib()
    dev = torch.device("cuda:0")
    mae = build_model(CFG2, "bf16", dev)
    sync = GradSync(mae)
    opt = FlatAdam(sync, lr=1e-4)
    torch.manual_seed(1234)
    x = synthetic_batch(CFG2, args.batch, dev)
    tf = mae.encoder.transformer

    def step():
        sync.zero_grad()
        loss = mae(x)
        loss.backward()
        sync.finish(defer_scale=True)
        opt.step()

    arms = {"a_default_p0": (False, 0.0), "b_default_p0.1": (False, 0.1), "c_perop_p0": (True, 0.0), "d_perop_p0.1": (True, 0.1)}
    times = {k: [] for k in arms}
    defaults = (lib.m3l_set_attn_block(3), lib.m3l_set_enc_mega(1), lib.m3l_set_t192(1))
    lib.m3l_set_attn_block(defaults[0]); lib.m3l_set_enc_mega(defaults[1]); lib.m3l_set_t192(defaults[2])
    for _ in range(args.rounds):
        for name, (perop, p) in arms.items():
            lib.m3l_set_attn_block(0 if perop else defaults[0])
            lib.m3l_set_enc_mega(0 if perop else defaults[1])
            lib.m3l_set_t192(0 if perop else defaults[2])
            tf.dropout_p = p
            for _ in range(args.warmup):
                step()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(args.steps):
                step()
            torch.cuda.synchronize()
            times[name].append((time.perf_counter() - t0) / args.steps * 1e3)
    lib.m3l_set_attn_block(defaults[0]); lib.m3l_set_enc_mega(defaults[1]); lib.m3l_set_t192(defaults[2])
    med = {k: round(statistics.median(v), 3) for k, v in times.items()}
    out = {"workload": "cfg2", "batch": args.batch, "dtype": "bf16", "ms_per_step_median": med, "ms_per_step_all": times,
           "d_over_c": round(med["d_perop_p0.1"] / med["c_perop_p0"], 4), "b_over_a": round(med["b_default_p0.1"] / med["a_default_p0"], 4)}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
