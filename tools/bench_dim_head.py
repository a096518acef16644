"""What a dim_head != 64 model pays for the per-op route (EXPERIMENTS.md "dim_head 32 / 128").

  1. attn_fwd / attn_bwd stand-alone at head width DH = 32 / 64 / 128, B = 256, n = 48 / 192, 3 heads, bf16: the in-library event
     brackets (m3l_prof_*), mean per launch over 20 launches after 3 warm-up launches.
  2. One cfg-2 training step (VTMAE forward + backward, ViT-Tiny 192 / 12 + decoder 192 / 4, B = 256, bf16) at dim_head = 32 (6 heads)
     and at dim_head = 64 (3 heads) with every fused block / row-tile / one-launch kernel switched off, so both run the per-op chain;
     and dim_head = 64 with the default kernel selection for comparison.  Mean over 10 steps after 3 warm-up steps (CUDA events).

Usage: python tools/bench_dim_head.py  (one JSON line on stdout)"""
import ctypes as C
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from m3l_amd import VTMAE, VTT  # noqa: E402
from m3l_amd import _lib as L  # noqa: E402

DEV = "cuda:0"


def _s():
    return torch.cuda.current_stream().cuda_stream


def _prof_classes():
    lib = L.lib()
    out = {}
    for i in range(lib.m3l_prof_count()):
        name = C.create_string_buffer(96)
        ms, n, w, b = C.c_double(), C.c_long(), C.c_double(), C.c_double()
        lib.m3l_prof_get(i, name, 96, C.byref(ms), C.byref(n), C.byref(w), C.byref(b))
        if n.value:
            out[name.value.decode()] = (ms.value / n.value * 1e3, w.value / n.value)
    return out


def attention():
    lib = L.lib()
    rows = []
    B, H = 256, 3
    for n in (48, 192):
        for DH in (32, 64, 128):
            qkv = torch.randn(B * n, 3 * H * DH, device=DEV).to(torch.bfloat16)
            o = torch.empty(B * n, H * DH, device=DEV, dtype=torch.bfloat16)
            dO = torch.randn(B * n, H * DH, device=DEV).to(torch.bfloat16)
            dqkv = torch.empty_like(qkv)
            lse = torch.empty(B, H, n, device=DEV)
            ds = torch.empty(B, H, n, device=DEV)

            def both():
                L.check(lib.m3l_op_attn_fwd_dh(1, L.ptr(qkv), L.ptr(o), L.ptr(lse), B, n, H, _s(), DH), "attn_fwd_dh")
                L.check(lib.m3l_op_attn_bwd_dh(1, L.ptr(qkv), L.ptr(o), L.ptr(dO), L.ptr(lse), L.ptr(ds), L.ptr(dqkv), B, n, H, _s(), DH),
                        "attn_bwd_dh")
            for _ in range(3):
                both()
            torch.cuda.synchronize()
            lib.m3l_prof_begin(None, 1)
            for _ in range(20):
                both()
            lib.m3l_prof_end()
            cls = _prof_classes()
            row = {"DH": DH, "B": B, "n": n, "H": H}
            for kind in ("attn_fwd", "attn_bwd"):
                (us, work), = [v for k, v in cls.items() if k.startswith(kind + "[")]
                row[kind + "_us"] = round(us, 1)
                row[kind + "_tflops"] = round(work / us / 1e6, 1)
            rows.append(row)
            print(json.dumps(row), file=sys.stderr)
    return rows


def step(dim_head, heads, per_op, B=256, steps=10, warm=3):
    lib = L.lib()
    olds = (lib.m3l_set_attn_block(0), lib.m3l_set_t192(0), lib.m3l_set_enc_mega(0)) if per_op else None
    try:
        torch.manual_seed(0)
        enc = VTT(image_size=64, tactile_size=32, image_patch_size=8, tactile_patch_size=4, dim=192, depth=12, heads=heads, mlp_dim=768,
                  dim_head=dim_head)
        mae = VTMAE(encoder=enc, decoder_dim=192, masking_ratio=0.75, decoder_depth=4, decoder_heads=heads, decoder_dim_head=dim_head,
                    compute_dtype="bf16").to(DEV)
        g = torch.Generator(device=DEV).manual_seed(1)
        x = {"image": torch.rand(B, 3, 64, 64, device=DEV, generator=g), "tactile1": torch.rand(B, 3, 32, 32, device=DEV, generator=g),
             "tactile2": torch.rand(B, 3, 32, 32, device=DEV, generator=g)}

        def one():
            mae.zero_grad(set_to_none=True)
            mae(x).backward()
        for _ in range(warm):
            one()
        torch.cuda.synchronize()
        lib.m3l_prof_begin(None, 1)
        one()
        lib.m3l_prof_end()
        fused = sorted(k for k in _prof_classes() if k.startswith(("attn_block_", "mlp_block_", "attn_t192_", "attn_tail_mlp_t192", "mlp_t192_",
                                                                    "qkv_bwd_t192", "enc_")))
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(steps):
            one()
        b.record()
        torch.cuda.synchronize()
        ms = a.elapsed_time(b) / steps
    finally:
        if olds:
            lib.m3l_set_attn_block(olds[0]), lib.m3l_set_t192(olds[1]), lib.m3l_set_enc_mega(olds[2])
    row = {"dim_head": dim_head, "heads": heads, "per_op_forced": per_op, "B": B, "ms_per_step": round(ms, 3),
           "samples_per_s": round(B / ms * 1e3, 1), "fused_kernel_classes": len(fused)}
    print(json.dumps(row), file=sys.stderr)
    return row


def main():
    res = {"attention": attention(),
           "cfg2_step": [step(32, 6, True), step(64, 3, True), step(64, 3, False)]}
    print(json.dumps(res))


if __name__ == "__main__":
    main()
