"""dim_head in {32, 64, 128}, host side: the modules construct with 32- / 128-wide heads exactly as vit-pytorch's Transformer does (keys,
shapes, seeded initial values), other widths are refused, and the oracle's `transformer` matches the reference-held fixtures of
tests/golden/make_golden_dim_head.py (the reference's own Block at head widths 32 and 128).  The GPU side is test_dim_head_gpu.py."""
import importlib.util
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
GOLDEN = os.path.join(ROOT, "tests", "golden")
if GOLDEN not in sys.path:
    sys.path.insert(0, GOLDEN)

import _thirdparty_restated as tp  # noqa: E402
from oracle import vtmae_oracle as O  # noqa: E402

KW = dict(image_size=32, tactile_size=16, image_patch_size=8, tactile_patch_size=4, dim=192, depth=2, heads=6, mlp_dim=384)


def _gen():
    spec = importlib.util.spec_from_file_location("make_golden_dim_head", os.path.join(GOLDEN, "make_golden_dim_head.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def _sd(model):
    return {k: v.detach().clone() for k, v in model.state_dict().items()}


def _same_state(a, b):
    sa, sb = _sd(a), _sd(b)
    assert list(sa) == list(sb)
    for k in sa:
        assert sa[k].shape == sb[k].shape and torch.equal(sa[k], sb[k]), k


@pytest.mark.parametrize("dim,heads,dim_head", [(192, 6, 32), (192, 3, 32), (256, 4, 128), (128, 1, 128), (128, 2, 64)])
def test_transformer_matches_vit_pytorch_at_seed(dim, heads, dim_head):
    from m3l_amd import Transformer
    torch.manual_seed(7)
    ours = Transformer(dim, 2, heads, dim_head, 2 * dim)
    torch.manual_seed(7)
    ref = tp.Transformer(dim, 2, heads, dim_head, 2 * dim)
    _same_state(ours, ref)
    inner = heads * dim_head
    assert ours.layers[0][0].to_qkv.weight.shape == (3 * inner, dim)
    assert ours.project_out == (not (heads == 1 and dim_head == dim))
    if ours.project_out:
        assert ours.layers[0][0].to_out[0].weight.shape == (dim, inner)
    else:
        assert isinstance(ours.layers[0][0].to_out, torch.nn.Identity)
    assert ours.layers[0][0].scale == dim_head ** -0.5
    cfg = ours._cfg()
    assert (cfg.dim, cfg.heads, cfg.dim_head, cfg.project_out) == (dim, heads, dim_head, int(ours.project_out))


@pytest.mark.parametrize("which", ["vtt", "vtmae", "dino"])
@pytest.mark.parametrize("dim_head", [32, 128])
def test_wrapping_modules_match_vit_pytorch_at_seed(monkeypatch, which, dim_head):
    """VTT(dim_head=…), VTMAE(decoder_dim_head=…) and DinoVTT(dim_head=…) under one seed equal the same modules built with vit-pytorch's
    Transformer in place of ours: the drop-in promise of the constructor kwargs."""
    import m3l_amd.dino_vtt as dv
    import m3l_amd.pretrain_models as pm
    from m3l_amd import VTMAE, VTT, DinoVTT

    def build():
        torch.manual_seed(11)
        if which == "vtt":
            return VTT(dim_head=dim_head, **KW)
        if which == "dino":
            return DinoVTT(dim_head=dim_head, **KW)
        return VTMAE(encoder=VTT(dim_head=dim_head, **KW), decoder_dim=128, decoder_depth=1, decoder_heads=3, decoder_dim_head=dim_head)

    ours = build()
    monkeypatch.setattr(pm, "Transformer", tp.Transformer)
    monkeypatch.setattr(dv, "Transformer", tp.Transformer)
    ref = build()
    _same_state(ours, ref)
    tf = ours.encoder.transformer if which == "vtmae" else ours.transformer
    assert tf.dim_head == dim_head and tf._cfg().dim_head == dim_head
    if which == "vtmae":
        assert ours.decoder.dim_head == dim_head and ours.decoder.layers[0][0].to_qkv.weight.shape == (3 * 3 * dim_head, 128)


@pytest.mark.parametrize("dim_head", [16, 48, 256])
def test_unsupported_dim_head_is_refused(dim_head):
    from m3l_amd import VTMAE, VTT, Transformer
    with pytest.raises(NotImplementedError, match=r"\(32, 64, 128\)"):
        Transformer(128, 1, 2, dim_head, 256)
    with pytest.raises(NotImplementedError, match=r"\(32, 64, 128\)"):
        VTT(dim_head=dim_head, **KW)
    with pytest.raises(NotImplementedError, match=r"\(32, 64, 128\)"):
        VTMAE(encoder=VTT(**KW), decoder_dim=128, decoder_depth=1, decoder_heads=2, decoder_dim_head=dim_head)


def test_tf_cfg_six_positional_values_mean_dim_head_64():
    from m3l_amd import _lib as L
    c = L.TfCfg(384, 12, 6, 1536, 1, 1)
    assert c.dim_head == 0            # 0 = 64 (include/m3l_amd.h m3l_tf_cfg)
    assert [f for f, _ in L.TfCfg._fields_][-1] == "dim_head"


def load_fixture(name):
    """-> (meta, params, {n: (x, cot)}, z) of a make_golden_dim_head fixture, its regenerated inputs checked against the recorded sums"""
    g = _gen()
    meta, params, data = g.stack_inputs(name)
    z = np.load(os.path.join(GOLDEN, name + ".npz"))
    assert [int(v) for v in z["meta"]] == [meta["D"], meta["depth"], meta["heads"], meta["mlp"], meta["dim_head"]]
    np.testing.assert_allclose([float(np.abs(v).astype(np.float64).sum()) for v in params.values()], z["check/param_abs_sum"], rtol=1e-12)
    for n, (x, _) in data.items():
        np.testing.assert_allclose(float(np.abs(x).astype(np.float64).sum()), float(z[f"n{n}/check/x_abs_sum"]), rtol=1e-12)
    return meta, params, data, z


@pytest.mark.parametrize("name", ["block_stack_dh32", "block_stack_dh128"])
@pytest.mark.parametrize("n", [48, 192])
def test_oracle_vs_reference_held_block_dim_head(name, n):
    """oracle.transformer at head widths 32 / 128 against the reference's OWN Block (same bounds as the block_stack.npz oracle test)."""
    meta, params, data, z = load_fixture(name)
    D, depth, heads, dh = meta["D"], meta["depth"], meta["heads"], meta["dim_head"]
    P = {"t." + k: torch.tensor(v).requires_grad_(True) for k, v in params.items()}
    x = torch.tensor(data[n][0]).requires_grad_(True)
    if n == 48:
        first = O.transformer(x, P, "t.", 1, heads, dh, final_norm=False)
        np.testing.assert_allclose(first.detach().numpy(), z[f"n{n}/block0_out"], rtol=1e-4, atol=1e-5)
    y = O.transformer(x, P, "t.", depth, heads, dh)
    np.testing.assert_allclose(y.detach().numpy(), z[f"n{n}/y"], rtol=1e-4, atol=1e-5)
    (y * torch.tensor(data[n][1])).sum().backward()
    np.testing.assert_allclose(x.grad.numpy(), z[f"n{n}/dx"], rtol=1e-3, atol=1e-5)
    for k, p in P.items():
        ref = z[f"n{n}/grad/" + k[2:]]
        got = p.grad.numpy()
        if got.ndim == 2:
            got = got[z["rows/" + k[2:]]]
        assert np.abs(got - ref).max() <= 1e-4 * np.abs(ref).max() + 1e-6, k
