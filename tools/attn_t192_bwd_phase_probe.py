#!/usr/bin/env python3
"""Where attn_t192_bwd spends its cycles, in both modes of m3l_set_attn_t192_bwd_prefetch: a diagnostic build (-DT192B_STAMP=1,
bash tools/t192_ablate.sh "1" t192 T192B_STAMP) accumulates shader-clock deltas per compute wave and phase; this prints their means
over the workgroups (and the fastest / slowest wave's mean), at the cfg-2 decoder shape (B = 256, n = 192, D = 192) and at D = 256.
usage: python tools/attn_t192_bwd_phase_probe.py build_abl/libt192_1.so      (env PB, PN: batch and sequence length)"""
import ctypes as C
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

lib = C.CDLL(sys.argv[1])
dev = "cuda:0"
B, n = int(os.environ.get("PB", "256")), int(os.environ.get("PN", "192"))
M = B * n
bf = torch.bfloat16
P = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
NAMES = ["kernel head (dx1_t requested)", "head 0: rows -> B0", "head 0: dO, Dsum, images -> B1", "head 0: query-owner pass",
         "head 0: key-owner pass, dqkv -> B2", "heads 1..: rows -> B0", "heads 1..: dO, Dsum, images -> B1", "heads 1..: query-owner pass",
         "heads 1..: key-owner pass, dqkv -> B2"]
for D in (192, 256):
    H = D // 64
    g = torch.Generator(device=dev).manual_seed(0)
    rn = lambda *s, dt=torch.float32, sc=1.0: (torch.randn(*s, device=dev, generator=g) * sc).to(dt)  # noqa: E731
    o, dxt, qkv = rn(M, D, dt=bf), rn(M, D, dt=bf), rn(M, 3 * D, dt=bf)
    lse = rn(B * H * n).abs() + 3.0
    woT = rn(D, D, dt=bf, sc=0.05)
    dqkv = torch.empty(M, 3 * D, device=dev, dtype=bf)
    stamps = torch.zeros(B * 12 * 16, dtype=torch.int64, device=dev)
    assert lib.m3l_t192b_set_stamps(P(stamps)) == 0
    fn = lambda: lib._Z17m3l_attn_t192_bwdiiiPKvS0_S0_PKfS0_PvP12ihipStream_t(  # noqa: E731
        D, B, n, P(dxt), P(qkv), P(o), P(lse), P(woT), P(dqkv), st)
    for mode, label in ((0, "rows by the compute waves"), (1, "rows by the DMA waves, one head ahead")):
        lib.m3l_set_attn_t192_bwd_prefetch(mode)
        for _ in range(5):
            assert fn() == 0
        torch.cuda.synchronize()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(20):
            fn()
        b.record()
        torch.cuda.synchronize()
        t = stamps.view(B, 12, 16).double().cpu()
        tot = t[:, :, :9].sum(2).mean().item()
        exposed = (t[:, :, 5] + t[:, :, 6]).mean().item()
        print(f"D {D} B {B} n {n} mode {mode} ({label}): instrumented {a.elapsed_time(b) / 20 * 1e3:.1f} us/launch; {tot:.0f} clock ticks per "
              f"compute wave; phases 1 + 2 of heads 1.. = {exposed / tot * 100:.1f} %", flush=True)
        for i, nm in enumerate(NAMES):
            w = t[:, :, i].mean(0)
            print(f"  {nm:38s} {t[:, :, i].mean().item():8.0f}  {t[:, :, i].mean().item() / tot * 100:5.1f} %   (wave means {w.min().item():7.0f} .. {w.max().item():7.0f})", flush=True)
    lib.m3l_t192b_set_stamps(None)
