"""Whole-model oracle parity with transformer dropout on: a cfg-2-shaped VTMAE(dropout=0.1) at full depth (12 encoder layers: the
backward's operand-set ring, and with it the masked-gradient buffers the side-stream weight gradients read, is reused) and M3L's default
architecture (EarlyCNN stems, early_conv_masking=True), fp32 and bf16, in train mode, against the CPU oracle (oracle/vtmae_oracle.py).
The oracle's transformer is replaced, inside the test, by a restatement that injects the masks of the header's generator (numpy,
test_dropout_cpu.py) keyed by the seed the encoder recorded; the decoder does not drop.  Bounds: those of the existing full-depth tests."""
import os
import sys

import pytest
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
from test_dropout_cpu import dropout_mask, keep_scale  # noqa: E402
from m3l_amd import VTMAE, VTT  # noqa: E402
from oracle import vtmae_oracle as O  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
P_DROP = 0.1
BF16_GTOL, BF16_L2TOL = 0.03, 6e-3          # tests/test_fulldepth_gpu.py


def _masked_transformer(seed, p, orig):
    """oracle.vtmae_oracle.transformer with vit-pytorch's four dropout sites on the encoder stack (prefix encoder.transformer.)"""
    s = keep_scale(p)

    def tf(x, P, prefix, depth, heads, dim_head, final_norm=True):
        if prefix != "encoder.transformer.":
            return orig(x, P, prefix, depth, heads, dim_head, final_norm)
        B, n, D = x.shape

        def m(layer, site, rows, N, shape):
            return torch.from_numpy(dropout_mask(p, seed, layer, site, rows, N)).to(x.dtype).reshape(shape) * s

        for i in range(depth):
            a = f"{prefix}layers.{i}.0."
            f = f"{prefix}layers.{i}.1.net."
            h = F.layer_norm(x, (D,), P[a + "norm.weight"], P[a + "norm.bias"], 1e-5)
            qkv = h @ P[a + "to_qkv.weight"].t()
            q, k, v = [t.reshape(B, n, heads, dim_head).transpose(1, 2) for t in qkv.chunk(3, dim=-1)]
            attn = ((q @ k.transpose(-1, -2)) * (dim_head ** -0.5)).softmax(dim=-1) * m(i, 0, B * heads * n, n, (B, heads, n, n))
            o = (attn @ v).transpose(1, 2).reshape(B, n, heads * dim_head)
            if (a + "to_out.0.weight") in P:
                o = (o @ P[a + "to_out.0.weight"].t() + P[a + "to_out.0.bias"]) * m(i, 1, B * n, D, (B, n, D))
            x = o + x
            h = F.layer_norm(x, (D,), P[f + "0.weight"], P[f + "0.bias"], 1e-5)
            mlp = P[f + "1.weight"].shape[0]
            h = F.gelu(h @ P[f + "1.weight"].t() + P[f + "1.bias"]) * m(i, 2, B * n, mlp, (B, n, mlp))
            x = (h @ P[f + "4.weight"].t() + P[f + "4.bias"]) * m(i, 3, B * n, D, (B, n, D)) + x
        if final_norm:
            x = F.layer_norm(x, (D,), P[prefix + "norm.weight"], P[prefix + "norm.bias"], 1e-5)
        return x
    return tf


def _run(monkeypatch, enc_kw, mae_kw, ocfg, B, C, hw, k, dt, ltol, gtol, l2tol):
    torch.manual_seed(0)
    mae = VTMAE(encoder=VTT(dropout=P_DROP, **enc_kw), compute_dtype=dt, **mae_kw).to(DEV)
    g = torch.Generator(device="cpu").manual_seed(99)
    with torch.no_grad():            # LayerNorm gains / biases and Linear biases away from 1 / 0 (every bias path matters)
        for prm in mae.parameters():
            if prm.dim() == 1:
                prm.add_((0.05 * torch.randn(prm.shape, generator=g)).to(prm.device))
    g = torch.Generator(device="cpu").manual_seed(1)
    x = {"image": torch.rand(B, C, hw[0], hw[0], generator=g)}
    for i in range(k):
        x[f"tactile{i + 1}"] = torch.rand(B, C, hw[1], hw[1], generator=g)
    noises = [torch.rand(B, ocfg.n_img, generator=g)] + [torch.rand(B, ocfg.n_tac, generator=g) for _ in range(k)]
    assert mae.training
    torch.manual_seed(5)
    loss = mae({kk: v.to(DEV) for kk, v in x.items()}, mask_noise=[n.to(DEV) for n in noises])
    loss.backward()
    torch.cuda.synchronize()
    seed = mae.encoder.transformer.last_dropout_seed
    assert seed is not None and mae.decoder.last_dropout_seed is None

    monkeypatch.setattr(O, "transformer", _masked_transformer(seed, P_DROP, O.transformer))
    P = {kk: v.detach().cpu().clone().requires_grad_(v.dtype.is_floating_point) for kk, v in mae.state_dict().items()}
    r = O.vtmae_forward(P, ocfg, x, noises)
    r["loss"].backward()
    assert torch.equal(mae.last_mask[0].cpu(), r["masked_indices"]) and torch.equal(mae.last_mask[1].cpu(), r["unmasked_indices"])
    rel = abs(float(loss.detach()) - float(r["loss"])) / abs(float(r["loss"]))
    num = den = 0.0
    worst = ("", 0.0)
    for name, prm in mae.named_parameters():
        ref = P[name].grad
        if ref is None:
            assert prm.grad is None, name
            continue
        assert prm.grad is not None, name
        d = prm.grad.cpu() - ref
        err = float(d.abs().max()) / max(1e-7, float(ref.abs().max()))
        if err > worst[1]:
            worst = (name, err)
        num += float(d.double().square().sum())
        den += float(ref.double().square().sum())
    l2 = (num / den) ** 0.5
    print(f"\n[dropout-oracle] dim {enc_kw['dim']} depth {enc_kw['depth']} {dt} B {B}: loss rel {rel:.2e}, worst grad {worst[0]} {worst[1]:.2e}, "
          f"grad rel-L2 {l2:.2e}")
    assert rel <= ltol, (rel, float(loss.detach()), float(r["loss"]))
    assert worst[1] <= gtol, (worst, l2)
    assert l2 <= l2tol, (l2, worst)
    # the masks mattered: without them the oracle's encoder output is far from the one the kernels matched (the loss alone moves little:
    # at initialisation it is dominated by the targets)
    monkeypatch.undo()
    P0 = {kk: v.detach().cpu().clone() for kk, v in mae.state_dict().items()}
    with torch.no_grad():
        e0, e1 = O.vtmae_forward(P0, ocfg, x, noises)["encoder_out"], r["encoder_out"].detach()
        assert float((e0 - e1).norm()) > 1e-2 * float(e1.norm()), float((e0 - e1).norm()) / float(e1.norm())


CFG2_ENC = dict(image_size=64, tactile_size=32, image_patch_size=8, tactile_patch_size=4, dim=192, depth=12, heads=3, mlp_dim=768)
CFG2_MAE = dict(decoder_dim=192, masking_ratio=0.75, decoder_depth=4, decoder_heads=3)
CFG2_O = O.OracleCfg(64, 32, 8, 4, 192, 12, 3, 768, 3, 2, 192, 4, 3, 0.75)


@pytest.mark.parametrize("dt", ["fp32", "bf16"])
def test_cfg2_full_depth_with_dropout_vs_oracle(monkeypatch, dt):
    """bounds of tests/test_fulldepth_gpu.py::test_cfg2_full_depth_vs_oracle at B = 16"""
    if dt == "fp32":
        _run(monkeypatch, CFG2_ENC, CFG2_MAE, CFG2_O, 16, 3, (64, 32), 2, dt, 1e-4, 2e-3, 1e-4)
    else:
        _run(monkeypatch, CFG2_ENC, CFG2_MAE, CFG2_O, 16, 3, (64, 32), 2, dt, 1e-2, BF16_GTOL, BF16_L2TOL)


REF_ENC = dict(image_size=64, tactile_size=32, image_patch_size=8, tactile_patch_size=4, dim=256, depth=4, heads=4, mlp_dim=512,
               image_channels=12, tactile_channels=12, num_tactiles=2, frame_stack=4)
REF_MAE = dict(decoder_dim=256, masking_ratio=0.95, decoder_depth=3, decoder_heads=4, num_tactiles=2, early_conv_masking=True, frame_stack=4)
REF_O = O.OracleCfg(64, 32, 8, 4, 256, 4, 4, 512, 12, 2, 256, 3, 4, 0.95)


# bounds of tests/test_parity_gpu.py::test_reference_default_architecture (per-parameter 1e-4 fp32; bf16 0.15 at B = 3, 0.05 at B = 40;
# whole-gradient rel-L2 1e-5 fp32 / 8e-3 bf16)
@pytest.mark.parametrize("dt,ltol,gtol,l2tol,B", [("fp32", 1e-4, 1e-4, 1e-5, 3), ("bf16", 1e-2, 0.15, 8e-3, 3), ("bf16", 1e-2, 0.05, 8e-3, 40)])
def test_reference_default_architecture_with_dropout_vs_oracle(monkeypatch, dt, ltol, gtol, l2tol, B):
    _run(monkeypatch, REF_ENC, REF_MAE, REF_O, B, 12, (64, 32), 2, dt, ltol, gtol, l2tol)
