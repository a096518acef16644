"""The cases of tests/test_tf_slices_gpu.py, the slices each tensor is cut into, the bound check, and the per-process caches of inputs and
references.  *** TEST INFRASTRUCTURE ONLY ***  The references and the input builder are in tests/tf_refs.py."""
import math
from dataclasses import dataclass
from typing import Optional

import torch

from tf_refs import EXACT, F64, recipe, run, tensors_of, trained_like

# -------------------------------------------------------------------------------------------------------------------
# the cases of tests/test_tf_slices_gpu.py.  sw: library switches (attn_block, t192, t192_tt, enc_mega, rowln); tile: height of the family's row
# tile; kt: key tile of the recipe (None: the per-sample attention of t192.hip runs at this shape)
@dataclass(frozen=True)
class Case:
    family: str
    D: int
    heads: int
    dim_head: int
    mlp: int
    n: int
    B: int
    depth: int
    recipe: str
    tile: int
    kt: Optional[int]
    sw: tuple                 # ((switch, value), ...)
    dtypes: tuple = ("bf16",)

    @property
    def id(self):
        return f"{self.family}-D{self.D}h{self.heads}x{self.dim_head}m{self.mlp}n{self.n}B{self.B}d{self.depth}"

    def inputs(self):
        return trained_like(self.D, self.depth, self.heads, self.dim_head, self.mlp, self.n, self.B, self.tile, seed=self.n + self.mlp)


def _cases():
    out = []
    off = (("attn_block", 0), ("t192", 0), ("rowln", 0))
    for j, (D, h, mlp, n, B) in enumerate([(192, 3, 768, 40, 3), (128, 2, 256, 17, 3), (192, 3, 768, 100, 2)]):
        for depth in ((2, 1) if j == 0 else (2,)):
            out.append(Case("perop", D, h, 64, mlp, n, B, depth, "perop", 64, 32, off, ("fp32", "bf16")))
    for D, h, dh, mlp, n, B in [(128, 4, 32, 256, 33, 3), (256, 2, 128, 512, 50, 2)]:
        out.append(Case("perop_dh", D, h, dh, mlp, n, B, 2, "perop", 64, 32, (), ("fp32", "bf16")))
    for mode in (1, 3):
        sw = (("attn_block", mode), ("t192", 0), ("rowln", 0), ("enc_mega", 0))
        for j, (D, h, mlp, n, B) in enumerate([(192, 3, 768, 48, 3), (192, 3, 64, 47, 2), (128, 2, 256, 33, 3), (128, 2, 128, 17, 3), (192, 3, 384, 1, 4)]):
            for depth in ((2, 1) if j == 0 else (2,)):
                out.append(Case(f"block{mode}", D, h, 64, mlp, n, B, depth, f"block{mode}", 16, 32, sw))
    for mega in (1, 2, 3):
        sw = (("attn_block", 3), ("t192", 0), ("rowln", 0), ("enc_mega", mega))
        for depth in (2, 5) + ((1,) if mega == 3 else ()):
            out.append(Case(f"mega{mega}", 192, 3, 64, 768, 48, 3, depth, "block3", 16, 32, sw))
    for tt in (12, 6):
        for j, (D, h, mlp, n, B) in enumerate([(192, 3, 768, 100, 3), (192, 3, 96, 64, 5), (192, 3, 384, 200, 2), (256, 4, 512, 75, 5), (384, 6, 768, 113, 3),
                                               (384, 4, 768, 75, 4)]):
            if tt == 6 and D != 192:
                continue                                       # (the tall-tile height is a D = 192 setting)
            tile = {192: 16 * tt, 256: 128, 384: 96}[D]
            kt = None if (D, h) in ((192, 3), (256, 4)) and 48 < n <= 192 else 32
            sw = (("attn_block", 1), ("t192", 7), ("t192_tt", tt), ("rowln", 0))
            for depth in ((2, 1) if (j == 0 and tt == 12) else (2,)):
                out.append(Case(f"rowtile_tt{tt}", D, h, 64, mlp, n, B, depth, "rowtile", tile, kt, sw))
    # the one large M (129 tiles of 192 rows: the library picks tall tiles from 128 up).  Depth 1: its float64 references are the file's whole cost
    out.append(Case("rowtile_auto", 192, 3, 64, 768, 192, 129, 1, "rowtile", 192, None, (("attn_block", 1), ("t192", 3), ("t192_tt", 12), ("rowln", 0))))
    for depth in (2, 1):
        out.append(Case("rowln", 192, 3, 64, 768, 40, 3, depth, "rowln", 64, 32, (("attn_block", 0), ("t192", 0), ("rowln", 1))))
    return out


CASES = _cases()


# -------------------------------------------------------------------------------------------------------------------
# slices
def slices(name, shape, case):
    """[(kind, label, index)] for tensor `name` ('y', 'dx' or a parameter name) of `shape`: the parts that are compared on their own"""
    H, dh, HD, n, B, tile = case.heads, case.dim_head, case.heads * case.dim_head, case.n, case.B, case.tile
    out = []
    if name in ("y", "dx"):                                     # (B, n, D): row tiles of the flattened matrix, first / last row of every sample
        M = B * n
        for r0 in range(0, M, tile):
            out.append(("rowtile", f"rows {r0}:{min(M, r0 + tile)}", ("flat", slice(r0, min(M, r0 + tile)))))
        for b in range(B):
            out.append(("sample_first", f"sample {b} row 0", (b, 0)))
            out.append(("sample_last", f"sample {b} row {n - 1}", (b, n - 1)))
    elif name.endswith("to_qkv.weight"):
        for j, part in enumerate("qkv"):
            for h in range(H):
                out.append((f"dW{part}", f"{part} head {h}", (slice(j * HD + h * dh, j * HD + (h + 1) * dh),)))
    elif name.endswith("to_out.0.weight"):
        for h in range(H):
            out.append(("dWo", f"head {h}", (slice(None), slice(h * dh, (h + 1) * dh))))
    elif name.endswith("net.1.weight") or name.endswith("net.1.bias"):
        for c in range(0, shape[0], 64):
            out.append(("dW1" if name.endswith("weight") else "db1", f"hidden {c}:{c + 64}", (slice(c, c + 64),)))
    elif name.endswith("net.4.weight"):
        for c in range(0, shape[1], 64):
            out.append(("dW2", f"hidden {c}:{c + 64}", (slice(None), slice(c, c + 64))))
    elif name.endswith("net.4.bias") or name.endswith("to_out.0.bias"):
        out.append(("dbias", "all", (slice(None),)))
    else:
        out.append(("ln", "all", (slice(None),)))
    return out


def take(t, index):
    if index[0] == "flat":
        return t.reshape(-1, t.shape[-1])[index[1]]
    return t[index]


SLICE_FLOOR = 1e-3       # max|X_slice| >= SLICE_FLOOR * max|X_tensor| for every slice (asserted on the CPU for every case)

# The one structural exception to the slice-scale condition, and the rule that replaces the relative bound there.  With n = 1 the softmax is
# the constant 1, so dS = P (dP - Dsum) and with it the q and k gradients are exactly 0 in X, R and F: the slice has no scale of its own and no
# input can give it one.  The kernels form dP (an MFMA) and Dsum (a lane sum) from the same dim_head products of bf16 values in two summation
# orders, so dP - Dsum is f32 summation noise, at most dim_head units of 2^-24 of the products' magnitude.  Those products are the ones the v
# gradient of the same tensor is made of (dV = P^T dO with P = 1), hence the bound: dim_head 2^-24 of the WHOLE tensor's largest exact element
# (3.8e-6 of it at dim_head 64; measured: 1e-8 to 3e-7, EXPERIMENTS 5.13).
def structural_zero(case, kind):
    return case.n == 1 and kind in ("dWq", "dWk")


def zero_slice_bound(case, x_tensor):
    return case.dim_head * 2.0 ** -24 * float(x_tensor.abs().max())


def check(case, got, X, Y, dt):
    """got / X / Y: tensors_of(...) of the HIP result, the exact reference and the yardstick (R for bf16, F for fp32).
    bf16: max|H - X|_s <= 2 max|R - X|_s + 2e-5 max|X|_s for every slice, and for slices of >= 1024 elements
          ||H - X||_s <= 1.5 ||R - X||_s + 2e-5 ||X||_s;  fp32: max|H - X|_s <= 4 max|F - X|_s + 1e-6 max|X|_s.
    The q / k slices of an n = 1 case: max|H|_s <= zero_slice_bound (see structural_zero above).
    -> (worst ratio per slice kind {kind: (ratio, tensor, label)}, list of failures); a ratio is error / bound, <= 1 passes"""
    fm, fl, floor = (2.0, 1.5, 2e-5) if dt == "bf16" else (4.0, None, 1e-6)
    worst, fails = {}, []
    for name, x in X.items():
        h, y = got[name].to(F64), Y[name].to(F64)
        for kind, label, idx in slices(name, x.shape, case):
            xs, eh, ey = take(x, idx), take(h - x, idx), take(y - x, idx)
            tests = [("max", float(eh.abs().max()), fm * float(ey.abs().max()) + floor * float(xs.abs().max()))]
            if structural_zero(case, kind):
                tests = [("max", tests[0][1], zero_slice_bound(case, x))]
            elif fl is not None and xs.numel() >= 1024:
                tests.append(("l2", float(eh.norm()), fl * float(ey.norm()) + floor * float(xs.norm())))
            for tk, e, bound in tests:
                ratio = e / bound if bound > 0 else (0.0 if e == 0 else math.inf)
                key = kind + ":" + tk
                if key not in worst or ratio > worst[key][0]:
                    worst[key] = (ratio, name, label)
                if not ratio <= 1.0:
                    fails.append((name, label, tk, e, bound))
    return worst, fails


# -------------------------------------------------------------------------------------------------------------------
# references of a case, computed once per process and never changed afterwards
_INPUTS, _REFS = {}, {}


def _input_key(case):
    return (case.D, case.heads, case.dim_head, case.mlp, case.n, case.B, case.depth, case.tile)


def inputs_of(case):
    k = _input_key(case)
    if k not in _INPUTS:
        _INPUTS[k] = case.inputs()
    return _INPUTS[k]


def reference(case, which, rb=False):
    """tensors_of(run(...)) for which = 'X' (exact), 'F' (float32) or 'R' (the case's recipe, with or without the bf16 residual stream)"""
    k = _input_key(case) + ((which,) if which != "R" else (which, case.recipe, case.kt, bool(rb)))
    if k not in _REFS:
        P, x, cot = inputs_of(case)
        rc = recipe(case.recipe, rb=rb, kt=case.kt) if which == "R" else EXACT
        res = run(x, cot, P, "", case.depth, case.heads, case.dim_head, rc, torch.float32 if which == "F" else F64)
        _REFS[k] = {name: t.to(F64) for name, t in tensors_of(res).items()}
    return _REFS[k]
