"""The default of m3l_set_drop_h, through the plan query and without a GPU: with the switch unset (auto) a stack stops saving h = GELU(u)
exactly where its forward feed-forward runs on a family of the measured set (EXPERIMENTS 5.36: the row tiles, i.e. the MAE decoder; the
per-sample blocks of the encoder keep h), per-op and dropout stacks always save it, and 0 / 1 still force both ways."""
import ctypes as C
import os

import pytest

from m3l_amd import _lib as L

AUTO = -1
ROW_TILES, BLOCKS = 1, 2            # the bits of m3l_set_drop_h_auto
DEFAULT_FAMILIES = ROW_TILES        # what section 5.36 measured as the better default


@pytest.fixture(autouse=True)
def _no_switch_in_the_environment():
    found = [v for v in ("M3L_DROP_H", "M3L_DROP_H_AUTO", "M3L_T192_MIN_TILES", "M3L_ROWTILE_MIN_ROWS") if v in os.environ]
    assert not found, f"unset {found}: this file states the defaults"


def S(D, depth, heads, mlp, dh=64):
    return L.TfCfg(D, depth, heads, mlp, 1, 1, dh)


ENC2, DEC2 = S(192, 12, 3, 768), S(192, 4, 3, 768)          # cfg 2 at B = 256: encoder over 48 visible tokens, decoder over all 192


def plan(cfg, B, n, p=0.0, drop_h=AUTO, families=None):
    lib, out = L.lib(), L.TfPlan()
    old = lib.m3l_set_drop_h(drop_h)
    old_f = lib.m3l_set_drop_h_auto(families) if families is not None else None
    try:
        drop = C.byref(L.Dropout(p, 7)) if p else None
        L.check(lib.m3l_transformer_plan(C.byref(cfg), B, n, drop, C.byref(out)), "m3l_transformer_plan")
    finally:
        if old_f is not None:
            lib.m3l_set_drop_h_auto(old_f)
        lib.m3l_set_drop_h(old)
    return out


def test_abi_version_and_the_unset_state():
    lib = L.lib()
    assert lib.m3l_version() >= 423
    old = lib.m3l_set_drop_h(AUTO)
    try:
        assert old == AUTO, "nothing has set the switch in this process: it reads auto"
        assert lib.m3l_set_drop_h(AUTO) == AUTO
        f = lib.m3l_set_drop_h_auto(DEFAULT_FAMILIES)
        assert f == DEFAULT_FAMILIES, "the built-in family mask is the measured default"
    finally:
        lib.m3l_set_drop_h(old)


def test_cfg2_plans_under_unset_switches():
    enc, dec = plan(ENC2, 256, 48), plan(DEC2, 256, 192)
    assert enc.fwd_mlp == L.TF_BLOCK and dec.fwd_mlp == L.TF_IN_TAIL
    assert (dec.drop_h, dec.h_from_u) == (1, 1), "the decoder's row tiles do not save h"
    want = 1 if DEFAULT_FAMILIES & BLOCKS else 0
    assert (enc.drop_h, enc.h_from_u) == (want, want)


@pytest.mark.parametrize("families", [0, ROW_TILES, BLOCKS, ROW_TILES | BLOCKS])
def test_auto_follows_the_family_mask(families):
    enc, dec = plan(ENC2, 256, 48, families=families), plan(DEC2, 256, 192, families=families)
    assert (enc.drop_h, enc.h_from_u) == ((1, 1) if families & BLOCKS else (0, 0))
    assert (dec.drop_h, dec.h_from_u) == ((1, 1) if families & ROW_TILES else (0, 0))
    # 48-row tiles on a short sequence (attention per op) are row tiles too
    short = plan(S(192, 4, 3, 768), 16, 192, families=families)
    assert short.fwd_mlp == L.TF_T192 and short.h_from_u == (1 if families & ROW_TILES else 0)


@pytest.mark.parametrize("drop_h", [AUTO, 0, 1])
def test_per_op_and_dropout_stacks_keep_h(drop_h):
    for cfg, B, n, p in ((ENC2, 256, 48, 0.1), (DEC2, 256, 192, 0.1), (S(192, 12, 6, 768, dh=32), 256, 48, 0.0),
                         (S(256, 4, 2, 1024, dh=128), 256, 192, 0.0), (S(384, 12, 6, 1536), 64, 113, 0.0)):
        o = plan(cfg, B, n, p, drop_h, families=ROW_TILES | BLOCKS)
        assert o.fwd_mlp == L.TF_PER_OP and o.h_from_u == 0
        assert o.drop_h == (1 if drop_h == 1 else 0), "auto never marks a stack whose fc2 GEMM reads h"


def test_zero_and_one_still_force():
    for cfg, B, n in ((ENC2, 256, 48), (DEC2, 256, 192)):
        off, on = plan(cfg, B, n, drop_h=0), plan(cfg, B, n, drop_h=1)
        assert (off.drop_h, off.h_from_u) == (0, 0) and (on.drop_h, on.h_from_u) == (1, 1)
    # the setter hands back what it replaced, auto included
    lib = L.lib()
    first = lib.m3l_set_drop_h(1)
    assert lib.m3l_set_drop_h(0) == 1 and lib.m3l_set_drop_h(AUTO) == 0 and lib.m3l_set_drop_h(first) == AUTO
