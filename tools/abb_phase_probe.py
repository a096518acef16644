#!/usr/bin/env python3
"""Where attn_block_bwd spends its cycles, per body (m3l_set_attn_bwd_heads 0 / 1): a diagnostic build (-DABB_STAMP=1,
bash tools/t192_ablate.sh "1" attn_block ABB_STAMP) accumulates shader-clock deltas per compute wave and phase; this prints their means
over the workgroups (and the fastest / slowest wave's mean), at the cfg-2 encoder shape.
usage: python tools/abb_phase_probe.py build_abl/libattn_block_1.so      (env PB, PN: batch and sequence length)"""
import ctypes as C
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

lib = C.CDLL(sys.argv[1])
dev = "cuda:0"
B, n, D = int(os.environ.get("PB", "256")), int(os.environ.get("PN", "48")), 192
M = B * n
g = torch.Generator(device=dev).manual_seed(0)
bf = torch.bfloat16
rn = lambda *s, dt=torch.float32, sc=1.0: (torch.randn(*s, device=dev, generator=g) * sc).to(dt)  # noqa: E731
x, dres, lw = rn(M, D), rn(M, D), rn(D, sc=0.1) + 1
o, dxt, qkv = rn(M, D, dt=bf), rn(M, D, dt=bf), rn(M, 3 * D, dt=bf)
lse = rn(B * 3 * n).abs() + 3.0
wqkvT, woT = rn(D, 3 * D, dt=bf, sc=0.05), rn(D, D, dt=bf, sc=0.05)
dqkv, dxo, dxt_o = torch.empty(M, 3 * D, device=dev, dtype=bf), torch.empty(M, D, device=dev), torch.empty(M, D, device=dev, dtype=bf)
ln_part = torch.empty(B, 3 * D, device=dev)
stamps = torch.zeros(B * 12 * 8, dtype=torch.int64, device=dev)
P = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
assert lib.m3l_abb_set_stamps(P(stamps)) == 0
fn = lambda: lib._Z18m3l_attn_block_bwdiiiPKvPKfS2_S2_S0_S0_S2_S0_S0_fPvPfS3_S4_P12ihipStream_t(  # noqa: E731
    D, B, n, P(dxt), P(dres), P(x), P(lw), P(qkv), P(o), P(lse), P(woT), P(wqkvT), C.c_float(1e-5), P(dqkv), P(dxo), P(dxt_o), P(ln_part), st)
NAMES = ["operands in -> B0", "dO -> X1", "Dsum -> X2", "attention backward -> X3", "dq|dk|dv / tiles in place, dqkv out", "dxn1 blocks", "tail"]
for mode, label in ((0, "per head"), (1, "all heads")):
    lib.m3l_set_attn_bwd_heads(mode)
    for _ in range(5):
        assert fn() == 0
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(20):
        fn()
    b.record()
    torch.cuda.synchronize()
    t = stamps.view(B, 12, 8).double().cpu()
    tot = t[:, :, :7].sum(2).mean().item()
    print(f"mode {mode} ({label}): instrumented {a.elapsed_time(b) / 20 * 1e3:.1f} us/launch; {tot:.0f} clock ticks per compute wave", flush=True)
    for i, nm in enumerate(NAMES):
        w = t[:, :, i].mean(0)
        print(f"  {nm:38s} {t[:, :, i].mean().item():8.0f}  {t[:, :, i].mean().item() / tot * 100:5.1f} %   (wave means {w.min().item():7.0f} .. {w.max().item():7.0f})", flush=True)
