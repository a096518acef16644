#!/usr/bin/env python3
"""Reference-held fixtures for attention heads that are not 64 wide (the generator runs ONLY in the build container, where the
reference is mounted; `stack_inputs` below is also what the tests import).

The reference's OWN pre-norm block (`tactile_ssl/model/layers/block.py` `Block`, loaded by make_golden._ref_layers) sets its head
width to dim // num_heads and scales q by head_dim ** -0.5, so choosing (dim, num_heads) chooses dim_head:

  block_stack_dh32.npz    D = 128, num_heads = 4  -> head width 32  (scale 0.1768)
  block_stack_dh128.npz   D = 256, num_heads = 2  -> head width 128 (scale 0.0884)

Each is produced as make_golden.run_block_stack produces block_stack.npz: a 2-layer stack + nn.LayerNorm at n = 48 and n = 192,
parameters mapped to vit-pytorch's Transformer names, output / input gradient / parameter gradients for a random cotangent.
To keep every file under 1 MiB the fixture does not store its inputs: parameters, tokens and cotangents come from `stack_inputs`, a
splitmix64 counter hash (plain numpy integer arithmetic, the same numbers on every machine), and the file records their sums as a
check.  Output, input gradient and every LayerNorm / bias gradient are stored whole, the output of layer 0 at n = 48; of each
weight gradient every ROW_STEP-th row (`rows/<name>` lists them).  `meta` = [D, depth, heads, mlp, dim_head].

Usage:  python tests/golden/make_golden_dim_head.py
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROW_STEP = 32
SHAPES = {"block_stack_dh32": dict(D=128, heads=4, mlp=256, seed=51, batches=((48, 3), (192, 2))),
          "block_stack_dh128": dict(D=256, heads=2, mlp=512, seed=61, batches=((48, 2), (192, 1)))}
DEPTH = 2


def _uniform(count, stream):
    """count floats uniform in [-1, 1) from a splitmix64 hash of (stream, index)."""
    with np.errstate(over="ignore"):
        z = np.arange(count, dtype=np.uint64) + np.uint64(stream) * np.uint64(0x9E3779B97F4A7C15)
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        z = z ^ (z >> np.uint64(31))
    return ((z >> np.uint64(40)).astype(np.float64) / float(1 << 23) - 1.0).astype(np.float32)


def param_shapes(D, heads, mlp):
    """vit-pytorch Transformer parameter names and shapes of the stack (dim_head = D // heads, to_out present)."""
    hd = D
    shapes = {}
    for i in range(DEPTH):
        shapes.update({f"layers.{i}.0.norm.weight": (D,), f"layers.{i}.0.norm.bias": (D,), f"layers.{i}.0.to_qkv.weight": (3 * hd, D),
                       f"layers.{i}.0.to_out.0.weight": (D, hd), f"layers.{i}.0.to_out.0.bias": (D,),
                       f"layers.{i}.1.net.0.weight": (D,), f"layers.{i}.1.net.0.bias": (D,), f"layers.{i}.1.net.1.weight": (mlp, D),
                       f"layers.{i}.1.net.1.bias": (mlp,), f"layers.{i}.1.net.4.weight": (D, mlp), f"layers.{i}.1.net.4.bias": (D,)})
    shapes.update({"norm.weight": (D,), "norm.bias": (D,)})
    return shapes


def stack_inputs(name):
    """-> (meta dict, params {name: float32 array}, {n: (x, cot)}) of fixture `name`: Linear weights uniform in +-1/sqrt(fan_in) (the
    scale of nn.Linear's init), LayerNorm weights 1 + 0.1 u, every 1-D parameter else 0.1 u, tokens 1.5 u sqrt(3), cotangents u sqrt(3)."""
    s = SHAPES[name]
    D, heads, mlp, seed = s["D"], s["heads"], s["mlp"], s["seed"]
    params = {}
    for j, (k, shp) in enumerate(param_shapes(D, heads, mlp).items()):
        u = _uniform(int(np.prod(shp)), seed * 1000 + j).reshape(shp)
        if len(shp) == 2:
            params[k] = (u / np.float32(np.sqrt(shp[1]))).astype(np.float32)
        elif k.endswith("norm.weight") or k.endswith("net.0.weight"):
            params[k] = (1.0 + 0.1 * u).astype(np.float32)
        else:
            params[k] = (0.1 * u).astype(np.float32)
    data = {}
    for j, (n, B) in enumerate(s["batches"]):
        x = (1.5 * np.sqrt(3.0) * _uniform(B * n * D, seed * 1000 + 500 + 2 * j)).astype(np.float32).reshape(B, n, D)
        cot = (np.sqrt(3.0) * _uniform(B * n * D, seed * 1000 + 501 + 2 * j)).astype(np.float32).reshape(B, n, D)
        data[n] = (x, cot)
    meta = dict(D=D, depth=DEPTH, heads=heads, mlp=mlp, dim_head=D // heads)
    return meta, params, data


def stored_rows(shape):
    """rows of a weight gradient the fixture keeps"""
    return np.arange(0, shape[0], ROW_STEP, dtype=np.int64)


def run_block_stack_dh(name):
    import torch
    sys.path.insert(0, HERE)
    import make_golden
    make_golden._load_reference()        # stubs + the reference on sys.path (what _ref_layers imports from)
    blk = make_golden._ref_layers()
    meta, params, data = stack_inputs(name)
    D, heads, mlp = meta["D"], meta["heads"], meta["mlp"]
    blocks = torch.nn.ModuleList([blk.Block(dim=D, num_heads=heads, mlp_ratio=mlp / D, qkv_bias=False) for _ in range(DEPTH)])
    norm = torch.nn.LayerNorm(D)
    assert blocks[0].attn.num_heads == heads and abs(blocks[0].attn.scale - meta["dim_head"] ** -0.5) < 1e-12
    assert blocks[0].mlp.fc1.weight.shape == (mlp, D)
    names = {}
    for i, b in enumerate(blocks):
        names.update({f"layers.{i}.0.norm.weight": b.norm1.weight, f"layers.{i}.0.norm.bias": b.norm1.bias,
                      f"layers.{i}.0.to_qkv.weight": b.attn.qkv.weight, f"layers.{i}.0.to_out.0.weight": b.attn.proj.weight,
                      f"layers.{i}.0.to_out.0.bias": b.attn.proj.bias, f"layers.{i}.1.net.0.weight": b.norm2.weight,
                      f"layers.{i}.1.net.0.bias": b.norm2.bias, f"layers.{i}.1.net.1.weight": b.mlp.fc1.weight,
                      f"layers.{i}.1.net.1.bias": b.mlp.fc1.bias, f"layers.{i}.1.net.4.weight": b.mlp.fc2.weight,
                      f"layers.{i}.1.net.4.bias": b.mlp.fc2.bias})
    names.update({"norm.weight": norm.weight, "norm.bias": norm.bias})
    assert len(names) == len(list(blocks.parameters())) + 2 and set(names) == set(params)
    with torch.no_grad():
        for k, p in names.items():
            p.copy_(torch.from_numpy(params[k]))
    out = {"meta": np.array([D, DEPTH, heads, mlp, meta["dim_head"]], dtype=np.int64),
           "check/param_abs_sum": np.array([float(np.abs(v).astype(np.float64).sum()) for v in params.values()])}
    for k, v in params.items():
        if v.ndim == 2:
            out["rows/" + k] = stored_rows(v.shape)
    for n, (xa, cota) in data.items():
        x = torch.from_numpy(xa).requires_grad_(True)
        cot = torch.from_numpy(cota)
        for p in names.values():
            p.grad = None
        h = x
        mids = []
        for b in blocks:
            h = b(h)
            mids.append(h)
        y = norm(h)
        (y * cot).sum().backward()
        out[f"n{n}/check/x_abs_sum"] = np.array(float(np.abs(xa).astype(np.float64).sum()))
        out[f"n{n}/y"], out[f"n{n}/dx"] = y.detach().numpy(), x.grad.numpy()
        if n == 48:
            out[f"n{n}/block0_out"] = mids[0].detach().numpy()
        for k, p in names.items():
            gr = p.grad.numpy()
            out[f"n{n}/grad/" + k] = gr[stored_rows(gr.shape)] if gr.ndim == 2 else gr.copy()
        print(f"{name} n={n}: y {tuple(y.shape)} |y| {float(y.detach().abs().mean()):.4f} scale {blocks[0].attn.scale:.4f}")
    path = os.path.join(HERE, name + ".npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


def main():
    for name in SHAPES:
        run_block_stack_dh(name)


if __name__ == "__main__":
    main()
