"""Transformer dropout, host side: a numpy restatement of the generator contract in include/m3l_amd.h ("Dropout") — Philox4x32-10
known answers, keep fraction, independence of sites / layers / seeds — and the modules' construction with dropout > 0.  The GPU
tests (test_dropout_gpu.py) pin the kernels to this restatement."""
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

_M0, _M1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)
_W0, _W1 = 0x9E3779B9, 0xBB67AE85
_LO = np.uint64(0xFFFFFFFF)


def philox4x32_10(ctr, key):
    """ctr: four uint32 arrays (broadcastable), key: (k0, k1) ints -> four uint32 arrays (Random123 word order)."""
    c0, c1, c2, c3 = (np.asarray(c, dtype=np.uint32) for c in ctr)
    k0, k1 = int(key[0]) & 0xFFFFFFFF, int(key[1]) & 0xFFFFFFFF
    for _ in range(10):
        p0 = c0.astype(np.uint64) * _M0
        p1 = c2.astype(np.uint64) * _M1
        hi0, lo0 = (p0 >> np.uint64(32)).astype(np.uint32), (p0 & _LO).astype(np.uint32)
        hi1, lo1 = (p1 >> np.uint64(32)).astype(np.uint32), (p1 & _LO).astype(np.uint32)
        c0, c1, c2, c3 = hi1 ^ c1 ^ np.uint32(k0), lo1, hi0 ^ c3 ^ np.uint32(k1), lo0
        k0, k1 = (k0 + _W0) & 0xFFFFFFFF, (k1 + _W1) & 0xFFFFFFFF
    return c0, c1, c2, c3


def _p32(p):
    """m3l_dropout.p is a float: the contract uses its float32 value, widened to double"""
    return np.float64(np.float32(p))


def threshold(p):
    return min(2 ** 32 - 1, int(np.floor(_p32(p) * 2.0 ** 32)))


def keep_scale(p):
    """the factor a kept element is multiplied by: (float)(1 / (1 - p)) in double, rounded once; p = 1 -> 0"""
    return 0.0 if _p32(p) >= 1.0 else float(np.float32(1.0 / (1.0 - _p32(p))))


def words(seed, layer, site, rows, N):
    """the Philox words of a (rows, N) site tensor: element (row, c) -> word c % 4 of block q = row ceil(N / 4) + c / 4"""
    nq = (N + 3) // 4
    q = np.arange(rows * nq, dtype=np.uint64)
    out = philox4x32_10((q & _LO, q >> np.uint64(32), np.full_like(q, 4 * layer + site), np.zeros_like(q)), (seed & 0xFFFFFFFF, seed >> 32))
    w = np.stack(out, axis=1).reshape(rows, nq * 4)
    return w[:, :N]


def dropout_mask(p, seed, layer, site, rows, N):
    """bool (rows, N): True = kept"""
    return words(seed, layer, site, rows, N) >= np.uint32(threshold(p))


def _hex(ws):
    return [f"{int(np.asarray(w).reshape(-1)[0]):08x}" for w in ws]


def test_philox_known_answers():
    assert _hex(philox4x32_10((0, 0, 0, 0), (0, 0))) == ["6627e8d5", "e169c58d", "bc57ac4c", "9b00dbd8"]
    f = 0xFFFFFFFF
    assert _hex(philox4x32_10((f, f, f, f), (f, f))) == ["408f276d", "41c83b0e", "a20bc7c6", "6d5451fd"]
    assert _hex(philox4x32_10((0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344), (0xA4093822, 0x299F31D0))) == \
        ["d16cfe09", "94fdcceb", "5001e420", "24126ea1"]


def test_threshold_and_scale_rules():
    assert threshold(0.0) == 0 and threshold(1.0) == 2 ** 32 - 1 and threshold(0.5) == 2 ** 31
    # p = 0.1 as float32 is 0.100000001490116...: T = floor(0.100000001490116 * 2^32) = 429496736, not the 429496729 of the double 0.1
    assert threshold(0.1) == 429496736
    assert keep_scale(0.1) == float(np.float32(1.0 / (1.0 - 0.10000000149011612))) and keep_scale(1.0) == 0.0
    assert dropout_mask(0.0, 5, 0, 0, 3, 7).all()


@pytest.mark.parametrize("p", [0.1, 0.5])
def test_keep_fraction(p):
    n = 0
    kept = 0
    for layer in range(3):             # 3 x 4 x 850,000 > 10^7 draws
        for site in range(4):
            m = dropout_mask(p, 0x1234_5678_9ABC_DEF0 + layer, layer, site, 8500, 100)
            kept += int(m.sum())
            n += m.size
    assert n >= 10 ** 7
    frac = kept / n
    sigma = (p * (1 - p) / n) ** 0.5
    assert abs(frac - (1 - p)) < 5 * sigma, (frac, 1 - p, sigma)


def test_sites_layers_seeds_uncorrelated():
    rows, N = 4000, 192
    seed = 987654321987654321
    ms = {"l0s1": dropout_mask(0.5, seed, 0, 1, rows, N), "l0s3": dropout_mask(0.5, seed, 0, 3, rows, N),
          "l1s1": dropout_mask(0.5, seed, 1, 1, rows, N), "seed+1": dropout_mask(0.5, seed + 1, 0, 1, rows, N),
          "seed_hi": dropout_mask(0.5, seed ^ (1 << 40), 0, 1, rows, N)}
    ref = ms.pop("l0s1").ravel().astype(np.float64)
    bound = 5.0 / ref.size ** 0.5
    for k, m in ms.items():
        c = np.corrcoef(ref, m.ravel().astype(np.float64))[0, 1]
        assert abs(c) < bound, (k, c, bound)


def test_ragged_row_length_groups_four_columns():
    # N not a multiple of 4: row r starts at block r * ceil(N / 4); the tail words of each row's last block are unused
    w = words(77, 2, 0, 3, 5)
    full = words(77, 2, 0, 3 * 2, 4).reshape(3, 8)
    assert np.array_equal(w, full[:, :5])


def _sd(model):
    return {k: v.detach().clone() for k, v in model.state_dict().items()}


@pytest.mark.parametrize("which", ["vtt", "vtmae", "dino"])
def test_modules_construct_with_dropout(which):
    from m3l_amd import VTMAE, VTT, DinoVTT
    kw = dict(image_size=32, tactile_size=16, image_patch_size=8, tactile_patch_size=4, dim=128, depth=2, heads=2, mlp_dim=256)

    def build(p):
        torch.manual_seed(3)
        if which == "vtt":
            return VTT(dropout=p, **kw)
        if which == "dino":
            return DinoVTT(dropout=p, **kw)
        return VTMAE(encoder=VTT(dropout=p, **kw), decoder_dim=128, decoder_depth=1, decoder_heads=2)

    a, b = build(0.0), build(0.1)
    sa, sb = _sd(a), _sd(b)
    assert list(sa) == list(sb)
    for k in sa:
        assert sa[k].shape == sb[k].shape and torch.equal(sa[k], sb[k]), k
    tf = b.encoder.transformer if which == "vtmae" else b.transformer
    assert tf.dropout_p == 0.1 and tf.last_dropout_seed is None
    if which == "vtmae":
        assert b.decoder.dropout_p == 0.0           # the decoder is built with dropout = 0, as in the reference


def test_dropout_descriptor_is_drawn_only_when_active():
    from m3l_amd.pretrain_models import Transformer
    tf = Transformer(128, 1, 2, 64, 256, dropout=0.25)
    tf.eval()
    assert tf._drop() is None
    tf.train()
    torch.manual_seed(9)
    d1 = tf._drop()
    torch.manual_seed(9)
    d2 = tf._drop()
    assert d1.seed == d2.seed == tf.last_dropout_seed and 0 <= d1.seed < 2 ** 63 and abs(d1.p - 0.25) < 1e-7
    assert Transformer(128, 1, 2, 64, 256)._drop() is None
    with pytest.raises(ValueError):
        Transformer(128, 1, 2, 64, 256, dropout=1.5)
