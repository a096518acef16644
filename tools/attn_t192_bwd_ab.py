#!/usr/bin/env python3
"""Stand-alone timing of attn_t192_bwd in both modes of m3l_set_attn_t192_bwd_prefetch, in alternating rounds of one process (and, when a
second library is given — a build of an older commit without the switch — that library's kernel as a third contestant in the same rounds),
at the cfg-2 decoder shape (D = 192, B = 256) and at M3L's default architecture (D = 256, B = 512), n = 192.  Checks first that the two
modes write the same bits.  Diagnostic only: calls the launcher by its mangled name, as tools/t192_probe.py does.
usage: python tools/attn_t192_bwd_ab.py [lib.so] [older_lib.so]      (env ROUNDS, default 7)"""
import ctypes as C
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402
from m3l_amd import _lib as L  # noqa: E402

libs = [a for a in sys.argv[1:] if a.endswith(".so")]
raw = C.CDLL(libs[0] if libs else L.LIB_PATH)
older = C.CDLL(libs[1]) if len(libs) > 1 else None
SYM = "_Z17m3l_attn_t192_bwdiiiPKvS0_S0_PKfS0_PvP12ihipStream_t"
dev = "cuda:0"
n = 192
bf = torch.bfloat16
P = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
st = C.c_void_p(torch.cuda.current_stream().cuda_stream)


def timed(fn, reps=20):
    for _ in range(3):
        assert fn() == 0
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / reps * 1e3


for D, B in ((192, 256), (256, 512)):
    H, M = D // 64, B * n
    g = torch.Generator(device=dev).manual_seed(0)
    rn = lambda *s, dt=torch.float32, sc=1.0: (torch.randn(*s, device=dev, generator=g) * sc).to(dt)  # noqa: E731
    o, dxt, qkv = rn(M, D, dt=bf), rn(M, D, dt=bf), rn(M, 3 * D, dt=bf)
    lse = rn(B * H * n).abs() + 3.0
    woT = rn(D, D, dt=bf, sc=0.05)
    dqkv = torch.empty(M, 3 * D, device=dev, dtype=bf)
    call = lambda lib: getattr(lib, SYM)(D, B, n, P(dxt), P(qkv), P(o), P(lse), P(woT), P(dqkv), st)  # noqa: E731
    old = raw.m3l_set_attn_t192_bwd_prefetch(0)
    bits = {}
    for mode in (0, 1):
        raw.m3l_set_attn_t192_bwd_prefetch(mode)
        dqkv.view(torch.uint8).fill_(0xFF)
        assert call(raw) == 0
        torch.cuda.synchronize()
        bits[mode] = dqkv.view(torch.uint8).clone()
    same = torch.equal(bits[0], bits[1])
    print(f"attn_t192_bwd D={D} B={B} n={n}: dqkv of the two modes bit-identical: {same}", flush=True)
    who = {"mode 0 (rows by the compute waves)": 0, "mode 1 (rows by the DMA waves)": 1}
    if older is not None:
        who["older library"] = None
    times = {k: [] for k in who}
    for _ in range(int(os.environ.get("ROUNDS", "7"))):
        for k, mode in who.items():
            if mode is None:
                times[k].append(timed(lambda: call(older)))
            else:
                raw.m3l_set_attn_t192_bwd_prefetch(mode)
                times[k].append(timed(lambda: call(raw)))
    raw.m3l_set_attn_t192_bwd_prefetch(old)
    for k in who:
        t = sorted(times[k])
        print(f"  {k:36s}: min {t[0]:6.1f}  median {t[len(t) // 2]:6.1f}  max {t[-1]:6.1f} us per launch over {len(t)} rounds", flush=True)
    assert same
