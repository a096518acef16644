"""The kernel selection of a transformer stack (m3l_transformer_plan, csrc/tf_plan.h) as a table, through the C ABI and without a GPU:
the plan is integer arithmetic on the configuration and the process-wide switches, and forward and backward launch what it says
(tests/test_tf_slices_gpu.py::test_plan_names_the_kernels_that_run checks that half on the device).

A row: the stack, B, n, the dropout rate, the switches that differ from the defaults below, and the expected plan as literals — the flags
that are set, the forward families (attention, out-proj, feed-forward), the backward families (feed-forward, attention, QKV), and
(row_tiles, qkv_tiles, cs_rows).  The expected values were produced by evaluating the conditions of the dispatcher this plan replaced, next
to the plan, over the grid of test_invariants_on_the_grid and more (EXPERIMENTS 5.14)."""
import ctypes as C
import itertools
import os

import pytest

import tf_cases as K
from m3l_amd import _lib as L

FAMILY = ["PER_OP", "BLOCK", "T192", "ROWLN", "IN_BLOCK", "TAIL_T192", "IN_TAIL", "GEMM", "IDENTITY"]       # the M3L_TF_* codes
FLAGS = ("per_op", "rowln_cfg", "rowln", "rb", "drop_h", "h_from_u", "mega_fwd", "mega_bwd", "dropout")
FWD, BWD = ("fwd_attn", "fwd_outproj", "fwd_mlp"), ("bwd_mlp", "bwd_attn", "bwd_qkv")
DEFAULTS = dict(attn_block=3, t192=1, t192_tt=12, enc_mega=1, rowln=0, residual_bf16=1, drop_h=0)
# tuning variables the library reads from the environment ONCE (function-local statics): a process that has one set computes another table
ENV_ONLY = ("M3L_T192_MIN_TILES", "M3L_ROWTILE_MIN_ROWS", "M3L_ROWTILE_384", "M3L_T192_ATTN", "M3L_WGRAD_LAYERS")


@pytest.fixture(autouse=True)
def _no_tuning_environment():
    found = [v for v in ENV_ONLY if v in os.environ]
    assert not found, f"unset {found}: the library caches them on first use and this table holds for their defaults only"


def S(D, depth, heads, mlp, dh=64, pout=1, dt=1):
    return L.TfCfg(D, depth, heads, mlp, pout, dt, dh)


def plan(cfg, B, n, p=0.0, sw=()):
    """the plan under DEFAULTS overlaid with sw; every switch is put back whatever happens"""
    lib, old, out = L.lib(), [], L.TfPlan()
    try:
        for name, v in dict(DEFAULTS, **dict(sw)).items():
            old.append((name, getattr(lib, "m3l_set_" + name)(v)))
        drop = C.byref(L.Dropout(p, 7)) if p else None
        L.check(lib.m3l_transformer_plan(C.byref(cfg), B, n, drop, C.byref(out)), "m3l_transformer_plan")
        assert out.rb == lib.m3l_transformer_rb(C.byref(cfg), B, n)
    finally:
        for name, v in reversed(old):
            getattr(lib, "m3l_set_" + name)(v)
    return out


def literal(o):
    return (" ".join(f for f in FLAGS if getattr(o, f)), " ".join(FAMILY[getattr(o, f)] for f in FWD), " ".join(FAMILY[getattr(o, f)] for f in BWD),
            (o.row_tiles, o.qkv_tiles, o.cs_rows))


ENC2, DEC2 = (192, 12, 3, 768), (192, 4, 3, 768)        # cfg 2 (the benchmark): encoder over the 48 visible tokens, decoder over all 192
ROWS = [
    ("cfg2 encoder", S(*ENC2), 256, 48, 0, {},
     "rb mega_fwd", "BLOCK IN_BLOCK BLOCK", "BLOCK BLOCK IN_BLOCK", (0, 0, 256)),
    ("cfg2 decoder B256", S(*DEC2), 256, 192, 0, {},
     "rb", "T192 TAIL_T192 IN_TAIL", "T192 T192 T192", (256, 256, 256)),
    ("cfg2 decoder B128", S(*DEC2), 128, 192, 0, {},
     "rb", "T192 TAIL_T192 IN_TAIL", "T192 T192 T192", (128, 128, 128)),
    # 16 tiles of 192 rows are fewer than t192_min_tiles: 48-row feed-forward tiles, everything else per-op
    ("cfg2 decoder B16", S(*DEC2), 16, 192, 0, {},
     "rb", "PER_OP GEMM T192", "T192 PER_OP PER_OP", (64, 0, 64)),
    # cfg 4: width 384 takes no row tiles by default; its 192-wide decoder at n = 452 has 151 tiles but too long a sequence for attn_t192
    ("cfg4 encoder visible", S(384, 12, 6, 1536), 64, 113, 0, {},
     "rb", "PER_OP GEMM PER_OP", "PER_OP PER_OP PER_OP", (0, 0, 57)),
    ("cfg4 encoder all tokens", S(384, 12, 6, 1536), 64, 452, 0, {},
     "rb", "PER_OP GEMM PER_OP", "PER_OP PER_OP PER_OP", (0, 0, 226)),
    ("cfg4 encoder n260", S(384, 12, 6, 1536), 64, 260, 0, {},
     "rb", "PER_OP GEMM PER_OP", "PER_OP PER_OP PER_OP", (0, 0, 130)),
    ("cfg4 decoder", S(192, 4, 3, 768), 64, 452, 0, {},
     "rb", "PER_OP TAIL_T192 IN_TAIL", "T192 PER_OP T192", (151, 151, 151)),
    ("cfg5 encoder", S(384, 4, 4, 768), 128, 15, 0, {},
     "rb", "PER_OP GEMM PER_OP", "PER_OP PER_OP PER_OP", (0, 0, 30)),
    ("cfg5 decoder", S(384, 3, 4, 1536), 128, 75, 0, {},
     "rb", "PER_OP GEMM PER_OP", "PER_OP PER_OP PER_OP", (0, 0, 75)),
    # M3L's default architecture at B = 512: 10 visible tokens; the decoder is M = 98 304 rows = 768 tiles of 128
    ("default encoder", S(256, 4, 4, 512), 512, 10, 0, {},
     "rb", "PER_OP GEMM PER_OP", "PER_OP PER_OP PER_OP", (0, 0, 80)),
    ("default decoder", S(256, 3, 4, 1024), 512, 192, 0, {},
     "rb", "T192 TAIL_T192 IN_TAIL", "T192 T192 T192", (768, 768, 6144)),
    # DinoVTT of the DINO step: 8 heads of 64 at width 256, so no out-proj prologue (HD != D) and no per-sample attention
    ("dino vtt", S(256, 4, 8, 512), 128, 194, 0, {},
     "rb", "PER_OP GEMM T192", "T192 PER_OP T192", (194, 194, 1552)),
    ("extractor head default", S(256, 1, 4, 512), 128, 192, 0, {},
     "rb", "T192 TAIL_T192 IN_TAIL", "T192 T192 T192", (192, 192, 1536)),
    ("extractor head cfg5", S(384, 1, 4, 768), 128, 75, 0, {},
     "rb", "PER_OP GEMM PER_OP", "PER_OP PER_OP PER_OP", (0, 0, 150)),
    ("cfg2 encoder fp32", S(*ENC2, dt=0), 256, 48, 0, {},
     "", "PER_OP GEMM PER_OP", "PER_OP PER_OP PER_OP", (0, 0, 96)),
    ("cfg2 decoder fp32", S(*DEC2, dt=0), 256, 192, 0, {},
     "", "PER_OP GEMM PER_OP", "PER_OP PER_OP PER_OP", (0, 0, 384)),
    ("dim_head 32", S(192, 12, 6, 768, dh=32), 256, 48, 0, {},
     "per_op rb", "PER_OP GEMM PER_OP", "PER_OP PER_OP PER_OP", (0, 0, 96)),
    ("dim_head 128", S(256, 4, 2, 1024, dh=128), 256, 192, 0, {},
     "per_op rb", "PER_OP GEMM PER_OP", "PER_OP PER_OP PER_OP", (0, 0, 384)),
    # dropout: per-op, and h is always saved there (the fc2 GEMM reads it), whatever drop_h says
    ("dropout encoder", S(*ENC2), 256, 48, 0.1, {"drop_h": 1},
     "per_op rb drop_h dropout", "PER_OP GEMM PER_OP", "PER_OP PER_OP PER_OP", (0, 0, 96)),
    ("dropout decoder", S(*DEC2), 256, 192, 0.1, {"drop_h": 1},
     "per_op rb drop_h dropout", "PER_OP GEMM PER_OP", "PER_OP PER_OP PER_OP", (0, 0, 384)),
    ("drop_h encoder", S(*ENC2), 256, 48, 0, {"drop_h": 1},
     "rb drop_h h_from_u mega_fwd", "BLOCK IN_BLOCK BLOCK", "BLOCK BLOCK IN_BLOCK", (0, 0, 256)),
    ("drop_h decoder", S(*DEC2), 256, 192, 0, {"drop_h": 1},
     "rb drop_h h_from_u", "T192 TAIL_T192 IN_TAIL", "T192 T192 T192", (256, 256, 256)),
    # to_out = Identity.  vit_pytorch makes it for heads == 1 and dim_head == dim only; neither width has a block kernel
    ("identity to_out 64", S(64, 2, 1, 256, pout=0), 256, 48, 0, {},
     "", "PER_OP IDENTITY PER_OP", "PER_OP PER_OP PER_OP", (0, 0, 192)),
    ("identity to_out 128", S(128, 2, 1, 256, dh=128, pout=0), 256, 48, 0, {},
     "per_op", "PER_OP IDENTITY PER_OP", "PER_OP PER_OP PER_OP", (0, 0, 192)),
    # ... the C ABI also takes project_out = 0 with heads * dim_head == dim.  The asymmetric row: the forward blocks need an out-projection
    # (per-op forward), the MLP block backward does not ask
    ("identity to_out 2 heads", S(128, 2, 2, 256, pout=0), 256, 48, 0, {},
     "", "PER_OP IDENTITY PER_OP", "BLOCK PER_OP PER_OP", (0, 0, 256)),
    ("enc_mega 0", S(*ENC2), 256, 48, 0, {"enc_mega": 0},
     "rb", "BLOCK IN_BLOCK BLOCK", "BLOCK BLOCK IN_BLOCK", (0, 0, 256)),
    ("enc_mega 1", S(*ENC2), 256, 48, 0, {"enc_mega": 1},
     "rb mega_fwd", "BLOCK IN_BLOCK BLOCK", "BLOCK BLOCK IN_BLOCK", (0, 0, 256)),
    # bit 2: the one-launch backward has no bf16-residual form
    ("enc_mega 2", S(*ENC2), 256, 48, 0, {"enc_mega": 2},
     "mega_bwd", "BLOCK IN_BLOCK BLOCK", "BLOCK BLOCK IN_BLOCK", (0, 0, 256)),
    ("enc_mega 3", S(*ENC2), 256, 48, 0, {"enc_mega": 3},
     "mega_fwd mega_bwd", "BLOCK IN_BLOCK BLOCK", "BLOCK BLOCK IN_BLOCK", (0, 0, 256)),
    # ... and refuses bf16 residuals even where mega_bwd turns out false for another reason (here: no attention backward block)
    ("enc_mega 2 attn_block 1", S(*ENC2), 256, 48, 0, {"enc_mega": 2, "attn_block": 1},
     "", "BLOCK IN_BLOCK BLOCK", "BLOCK PER_OP PER_OP", (0, 0, 256)),
    ("one launch holds 16 layers", S(192, 17, 3, 768), 256, 48, 0, {},
     "rb", "BLOCK IN_BLOCK BLOCK", "BLOCK BLOCK IN_BLOCK", (0, 0, 256)),
    ("rowln encoder", S(*ENC2), 256, 48, 0, {"rowln": 1},
     "rowln_cfg rowln", "PER_OP ROWLN ROWLN", "ROWLN PER_OP ROWLN", (0, 0, 96)),
    ("rowln decoder", S(*DEC2), 256, 192, 0, {"rowln": 1},
     "rowln_cfg rowln", "PER_OP ROWLN ROWLN", "ROWLN PER_OP ROWLN", (0, 0, 384)),
    ("rowln too wide", S(384, 4, 6, 1536), 64, 113, 0, {"rowln": 1},
     "rb", "PER_OP GEMM PER_OP", "PER_OP PER_OP PER_OP", (0, 0, 57)),
    # a per-op stack with the switch set runs no epilogue kernel, and keeps fp32 residuals all the same
    ("rowln dim_head 32", S(192, 12, 6, 768, dh=32), 256, 48, 0, {"rowln": 1},
     "per_op rowln_cfg", "PER_OP GEMM PER_OP", "PER_OP PER_OP PER_OP", (0, 0, 96)),
    ("fp32 residuals", S(*DEC2), 256, 192, 0, {"residual_bf16": 0},
     "", "T192 TAIL_T192 IN_TAIL", "T192 T192 T192", (256, 256, 256)),
    # t192 bit 2: the row tiles take the MLP halves of short sequences, so no MLP block and with it no attention backward block
    ("t192 short", S(*ENC2), 256, 48, 0, {"t192": 3},
     "rb", "BLOCK IN_BLOCK T192", "T192 PER_OP PER_OP", (256, 0, 256)),
    ("attn_block 1", S(*ENC2), 256, 48, 0, {"attn_block": 1},
     "rb mega_fwd", "BLOCK IN_BLOCK BLOCK", "BLOCK PER_OP PER_OP", (0, 0, 256)),
    ("attn_block off", S(*ENC2), 256, 48, 0, {"attn_block": 0},
     "rb", "PER_OP GEMM T192", "T192 PER_OP PER_OP", (256, 0, 256)),
    ("width 384 forced", S(384, 2, 6, 1536), 64, 113, 0, {"t192": 7},
     "rb", "PER_OP TAIL_T192 IN_TAIL", "T192 PER_OP T192", (76, 76, 456)),
]

# every Case of tests/tf_cases.py in bf16 under its own switches
CASE_ROWS = {
    "perop-D192h3x64m768n40B3d2": ("rb", "PER_OP GEMM PER_OP", "PER_OP PER_OP PER_OP", (0, 0, 2)),
    "perop-D192h3x64m768n40B3d1": ("rb", "PER_OP GEMM PER_OP", "PER_OP PER_OP PER_OP", (0, 0, 2)),
    "perop-D128h2x64m256n17B3d2": ("rb", "PER_OP GEMM PER_OP", "PER_OP PER_OP PER_OP", (0, 0, 1)),
    "perop-D192h3x64m768n100B2d2": ("rb", "PER_OP GEMM PER_OP", "PER_OP PER_OP PER_OP", (0, 0, 4)),
    "perop_dh-D128h4x32m256n33B3d2": ("per_op rb", "PER_OP GEMM PER_OP", "PER_OP PER_OP PER_OP", (0, 0, 2)),
    "perop_dh-D256h2x128m512n50B2d2": ("per_op rb", "PER_OP GEMM PER_OP", "PER_OP PER_OP PER_OP", (0, 0, 2)),
    "block1-D192h3x64m768n48B3d2": ("rb", "BLOCK IN_BLOCK BLOCK", "BLOCK PER_OP PER_OP", (0, 0, 3)),
    "block1-D192h3x64m768n48B3d1": ("rb", "BLOCK IN_BLOCK BLOCK", "BLOCK PER_OP PER_OP", (0, 0, 3)),
    "block1-D192h3x64m64n47B2d2": ("rb", "BLOCK IN_BLOCK BLOCK", "BLOCK PER_OP PER_OP", (0, 0, 2)),
    "block1-D128h2x64m256n33B3d2": ("rb", "BLOCK IN_BLOCK BLOCK", "BLOCK PER_OP PER_OP", (0, 0, 3)),
    "block1-D128h2x64m128n17B3d2": ("rb", "BLOCK IN_BLOCK BLOCK", "BLOCK PER_OP PER_OP", (0, 0, 3)),
    "block1-D192h3x64m384n1B4d2": ("rb", "BLOCK IN_BLOCK BLOCK", "BLOCK PER_OP PER_OP", (0, 0, 4)),
    "block3-D192h3x64m768n48B3d2": ("rb", "BLOCK IN_BLOCK BLOCK", "BLOCK BLOCK IN_BLOCK", (0, 0, 3)),
    "block3-D192h3x64m768n48B3d1": ("rb", "BLOCK IN_BLOCK BLOCK", "BLOCK BLOCK IN_BLOCK", (0, 0, 3)),
    "block3-D192h3x64m64n47B2d2": ("rb", "BLOCK IN_BLOCK BLOCK", "BLOCK BLOCK IN_BLOCK", (0, 0, 2)),
    "block3-D128h2x64m256n33B3d2": ("rb", "BLOCK IN_BLOCK BLOCK", "BLOCK BLOCK IN_BLOCK", (0, 0, 3)),
    "block3-D128h2x64m128n17B3d2": ("rb", "BLOCK IN_BLOCK BLOCK", "BLOCK BLOCK IN_BLOCK", (0, 0, 3)),
    "block3-D192h3x64m384n1B4d2": ("rb", "BLOCK IN_BLOCK BLOCK", "BLOCK BLOCK IN_BLOCK", (0, 0, 4)),
    "mega1-D192h3x64m768n48B3d2": ("rb mega_fwd", "BLOCK IN_BLOCK BLOCK", "BLOCK BLOCK IN_BLOCK", (0, 0, 3)),
    "mega1-D192h3x64m768n48B3d5": ("rb mega_fwd", "BLOCK IN_BLOCK BLOCK", "BLOCK BLOCK IN_BLOCK", (0, 0, 3)),
    "mega2-D192h3x64m768n48B3d2": ("mega_bwd", "BLOCK IN_BLOCK BLOCK", "BLOCK BLOCK IN_BLOCK", (0, 0, 3)),
    "mega2-D192h3x64m768n48B3d5": ("mega_bwd", "BLOCK IN_BLOCK BLOCK", "BLOCK BLOCK IN_BLOCK", (0, 0, 3)),
    "mega3-D192h3x64m768n48B3d2": ("mega_fwd mega_bwd", "BLOCK IN_BLOCK BLOCK", "BLOCK BLOCK IN_BLOCK", (0, 0, 3)),
    "mega3-D192h3x64m768n48B3d5": ("mega_fwd mega_bwd", "BLOCK IN_BLOCK BLOCK", "BLOCK BLOCK IN_BLOCK", (0, 0, 3)),
    "mega3-D192h3x64m768n48B3d1": ("mega_fwd mega_bwd", "BLOCK IN_BLOCK BLOCK", "BLOCK BLOCK IN_BLOCK", (0, 0, 3)),
    "rowtile_tt12-D192h3x64m768n100B3d2": ("rb", "T192 TAIL_T192 IN_TAIL", "T192 T192 T192", (2, 2, 2)),
    "rowtile_tt12-D192h3x64m768n100B3d1": ("rb", "T192 TAIL_T192 IN_TAIL", "T192 T192 T192", (2, 2, 2)),
    "rowtile_tt12-D192h3x64m96n64B5d2": ("", "T192 TAIL_T192 IN_TAIL", "T192 T192 T192", (2, 2, 2)),          # (mlp 96: no whole K tile for the residual epilogue)
    "rowtile_tt12-D192h3x64m384n200B2d2": ("rb", "PER_OP TAIL_T192 IN_TAIL", "T192 PER_OP T192", (3, 3, 3)),
    "rowtile_tt12-D256h4x64m512n75B5d2": ("rb", "T192 TAIL_T192 IN_TAIL", "T192 T192 T192", (3, 3, 24)),
    "rowtile_tt12-D384h6x64m768n113B3d2": ("rb", "PER_OP TAIL_T192 IN_TAIL", "T192 PER_OP T192", (4, 4, 24)),
    "rowtile_tt12-D384h4x64m768n75B4d2": ("rb", "PER_OP GEMM T192", "T192 PER_OP T192", (4, 4, 24)),
    "rowtile_tt6-D192h3x64m768n100B3d2": ("rb", "T192 TAIL_T192 IN_TAIL", "T192 T192 T192", (4, 4, 24)),
    "rowtile_tt6-D192h3x64m96n64B5d2": ("", "T192 TAIL_T192 IN_TAIL", "T192 T192 T192", (4, 4, 24)),
    "rowtile_tt6-D192h3x64m384n200B2d2": ("rb", "PER_OP TAIL_T192 IN_TAIL", "T192 PER_OP T192", (5, 5, 30)),
    "rowtile_auto-D192h3x64m768n192B129d1": ("rb", "T192 TAIL_T192 IN_TAIL", "T192 T192 T192", (129, 129, 129)),
    "rowln-D192h3x64m768n40B3d2": ("rowln_cfg rowln", "PER_OP ROWLN ROWLN", "ROWLN PER_OP ROWLN", (0, 0, 2)),
    "rowln-D192h3x64m768n40B3d1": ("rowln_cfg rowln", "PER_OP ROWLN ROWLN", "ROWLN PER_OP ROWLN", (0, 0, 2)),
}


def test_abi_version_has_the_plan_query():
    assert L.lib().m3l_version() >= 408


@pytest.mark.parametrize("row", ROWS, ids=lambda r: r[0].replace(" ", "_"))
def test_plan_table(row):
    _, cfg, B, n, p, sw, *want = row
    assert literal(plan(cfg, B, n, p, sw)) == tuple(want)


def test_every_slice_case_is_in_the_table():
    assert set(CASE_ROWS) == {c.id for c in K.CASES}


@pytest.mark.parametrize("case", K.CASES, ids=lambda c: c.id)
def test_plan_of_the_slice_cases(case):
    got = literal(plan(S(case.D, case.depth, case.heads, case.mlp, dh=case.dim_head), case.B, case.n, 0, case.sw))
    assert got == CASE_ROWS[case.id]


def test_a_refused_configuration_is_an_error_not_a_plan():
    out = L.TfPlan()
    assert L.lib().m3l_transformer_plan(C.byref(S(192, 2, 3, 768, dh=48)), 4, 48, None, C.byref(out)) == 1
    assert "dim_head" in L.last_error()
    assert L.lib().m3l_transformer_plan(C.byref(S(192, 2, 3, 768)), 0, 48, None, C.byref(out)) == 1


def check_invariants(o, cfg):
    fam = {f: FAMILY[getattr(o, f)] for f in FWD + BWD}
    fused_mlp = ("BLOCK", "T192", "IN_TAIL")
    if o.mega_fwd:
        assert fam["fwd_attn"] == "BLOCK" and fam["fwd_mlp"] == "BLOCK"
    if o.per_op:
        assert set(fam.values()) <= {"PER_OP", "GEMM", "IDENTITY"} and not o.rowln
    assert (fam["fwd_outproj"] == "TAIL_T192") == (fam["fwd_mlp"] == "IN_TAIL")
    assert (fam["fwd_outproj"] == "IN_BLOCK") == (fam["fwd_attn"] == "BLOCK")
    assert (fam["fwd_outproj"] == "IDENTITY") == (not cfg.project_out)
    if fam["bwd_attn"] == "BLOCK":
        assert fam["bwd_mlp"] == "BLOCK"
    assert (fam["bwd_qkv"] == "IN_BLOCK") == (fam["bwd_attn"] == "BLOCK")
    assert o.h_from_u == (o.drop_h and not o.per_op and fam["fwd_mlp"] in fused_mlp)
    if o.rb:
        assert cfg.dtype == 1 and not o.rowln_cfg and not o.mega_bwd
    if o.mega_bwd:
        assert fam["bwd_mlp"] == "BLOCK" and fam["bwd_attn"] == "BLOCK"
    assert o.rowln == (o.rowln_cfg and not o.per_op)
    if o.rowln:
        assert set(fam.values()) <= {"PER_OP", "ROWLN", "IDENTITY"} and fam["fwd_mlp"] == fam["bwd_mlp"] == fam["bwd_qkv"] == "ROWLN"
    if cfg.dtype == 0:
        assert set(fam.values()) <= {"PER_OP", "ROWLN", "GEMM", "IDENTITY"} and not o.rb and not o.mega_fwd and not o.mega_bwd
    assert (o.row_tiles > 0) == (fam["bwd_mlp"] == "T192") and (o.qkv_tiles > 0) == (fam["bwd_qkv"] == "T192") and o.cs_rows > 0


def test_invariants_on_the_table():
    for _, cfg, B, n, p, sw, *_ in ROWS:
        check_invariants(plan(cfg, B, n, p, sw), cfg)


# the switch settings of the rows and cases above, each against every shape of the grid
SETTINGS = sorted({tuple(sorted(r[5].items())) for r in ROWS} | {tuple(sorted(c.sw)) for c in K.CASES})


@pytest.mark.parametrize("sw", SETTINGS, ids=lambda s: "-".join(f"{k}{v}" for k, v in s) or "defaults")
def test_invariants_on_the_grid(sw):
    lib, old, out, drop = L.lib(), [], L.TfPlan(), L.Dropout(0.1, 7)
    try:
        for name, v in dict(DEFAULTS, **dict(sw)).items():
            old.append((name, getattr(lib, "m3l_set_" + name)(v)))
        for dt, D, dh, mlp in itertools.product((0, 1), (64, 128, 192, 256, 384, 512), (32, 64, 128), (64, 96, 768, 2048, 4096)):
            heads = max(1, D // dh)
            cfg = S(D, 2, heads, mlp, dh=dh, pout=0 if (heads == 1 and dh == D) else 1, dt=dt)
            for n, B, dp in itertools.product((1, 17, 48, 49, 192, 193, 452), (1, 3, 128, 256), (None, drop)):
                assert lib.m3l_transformer_plan(C.byref(cfg), B, n, dp, C.byref(out)) == 0
                assert out.rb == lib.m3l_transformer_rb(C.byref(cfg), B, n) and out.dropout == (dp is not None)
                check_invariants(out, cfg)
    finally:
        for name, v in reversed(old):
            getattr(lib, "m3l_set_" + name)(v)
