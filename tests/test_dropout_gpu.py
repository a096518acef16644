"""Transformer dropout on the MI355X: the in-kernel masks equal the numpy restatement of the header's generator bit for bit, a stack
with dropout matches a float64 torch restatement with those masks injected (output, input gradient, every parameter gradient), the
fused MAE step / extractor equal the per-module chains bit for bit with dropout on, and the train / eval rule of nn.Dropout holds."""
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
from test_dropout_cpu import dropout_mask, keep_scale  # noqa: E402
from m3l_amd import VTMAE, VTT  # noqa: E402
from m3l_amd import _lib as L  # noqa: E402
from m3l_amd import functional as Fn  # noqa: E402
from m3l_amd.pretrain_models import Transformer  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
P_DROP = 0.1


def _gpu_mask(p, seed, layer, site, rows, N):
    out = torch.empty(rows, N, dtype=torch.uint8, device=DEV)
    L.check(L.lib().m3l_op_dropout_mask(p, seed, layer, site, rows, N, L.ptr(out), Fn._stream()), "m3l_op_dropout_mask")
    torch.cuda.synchronize()
    return out.cpu().numpy().astype(bool)


@pytest.mark.parametrize("rows,N", [(4 * 3 * 48, 48), (2 * 3 * 192, 192), (2 * 6 * 113, 113), (4 * 48, 192), (2 * 113, 768),
                                    (4 * 48, 128), (7, 5)])
def test_mask_kernel_equals_restatement(rows, N):
    seed = 0x0123_4567_89AB_CDEF
    for p, layer, site in [(P_DROP, 0, 0), (P_DROP, 1, 3), (0.5, 5, 2), (1.0, 0, 1)]:
        assert np.array_equal(_gpu_mask(p, seed, layer, site, rows, N), dropout_mask(p, seed, layer, site, rows, N)), (p, layer, site)


def _ref_stack(x, P, depth, heads, seed, p, project_out):
    """vit_pytorch Transformer forward in float64 with the contract's masks injected at the four sites"""
    B, n, D = x.shape
    s = keep_scale(p)

    def m(layer, site, rows, N, shape):
        return torch.from_numpy(dropout_mask(p, seed, layer, site, rows, N)).double().reshape(shape) * s

    for i in range(depth):
        a, f = f"layers.{i}.0.", f"layers.{i}.1.net."
        h = F.layer_norm(x, (D,), P[a + "norm.weight"], P[a + "norm.bias"], 1e-5)
        q, k, v = [t.reshape(B, n, heads, 64).transpose(1, 2) for t in (h @ P[a + "to_qkv.weight"].t()).chunk(3, dim=-1)]
        attn = ((q @ k.transpose(-1, -2)) * 0.125).softmax(dim=-1) * m(i, 0, B * heads * n, n, (B, heads, n, n))
        o = (attn @ v).transpose(1, 2).reshape(B, n, heads * 64)
        if project_out:
            o = (o @ P[a + "to_out.0.weight"].t() + P[a + "to_out.0.bias"]) * m(i, 1, B * n, D, (B, n, D))
        x = o + x
        h = F.layer_norm(x, (D,), P[f + "0.weight"], P[f + "0.bias"], 1e-5)
        mlp = P[f + "1.weight"].shape[0]
        h = F.gelu(h @ P[f + "1.weight"].t() + P[f + "1.bias"]) * m(i, 2, B * n, mlp, (B, n, mlp))
        x = (h @ P[f + "4.weight"].t() + P[f + "4.bias"]) * m(i, 3, B * n, D, (B, n, D)) + x
    return F.layer_norm(x, (D,), P["norm.weight"], P["norm.bias"], 1e-5)


def _rel(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return float((a - b).abs().max()) / max(1e-12, float(b.abs().max())), float((a - b).norm()) / max(1e-30, float(b.norm()))


CASES = [  # (D, heads, n, B, mlp)
    (192, 3, 48, 4, 384),        # encoder shape
    (192, 3, 192, 2, 384),
    (384, 6, 113, 2, 768),       # cfg-4 encoder
    (64, 1, 48, 4, 128),         # heads = 1, dim = 64: to_out is Identity (no site 1)
]


@pytest.mark.parametrize("case", CASES)
@pytest.mark.parametrize("mode", ["fp32", "bf16", "bf16_res32"])
def test_stack_matches_float64_restatement(case, mode):
    D, heads, n, B, mlp = case
    depth = 2
    torch.manual_seed(5)
    tf = Transformer(D, depth, heads, 64, mlp, dropout=P_DROP).to(DEV)
    with torch.no_grad():              # non-trivial LayerNorm / bias parameters
        for name, prm in tf.named_parameters():
            if "norm" in name or name.endswith("bias"):
                prm.add_(0.1 * torch.randn_like(prm))
    tf.compute_dtype = "fp32" if mode == "fp32" else "bf16"
    tf.train()
    g = torch.Generator(device="cpu").manual_seed(6)
    x = torch.randn(B, n, D, generator=g)
    w = torch.randn(B, n, D, generator=g)
    xd = x.to(DEV).requires_grad_(True)
    old = L.lib().m3l_set_residual_bf16(0) if mode == "bf16_res32" else None
    try:
        y = tf(xd)
        (y * w.to(DEV)).sum().backward()
        torch.cuda.synchronize()
    finally:
        if old is not None:
            L.lib().m3l_set_residual_bf16(old)
    seed = tf.last_dropout_seed
    P = {k: v.detach().double().cpu().requires_grad_(True) for k, v in tf.named_parameters()}
    xr = x.double().requires_grad_(True)
    yr = _ref_stack(xr, P, depth, heads, seed, P_DROP, tf.project_out)
    (yr * w.double()).sum().backward()
    assert len(P) == 11 * depth + 2 - (0 if tf.project_out else 2 * depth)
    pairs = [("y", y.detach(), yr.detach()), ("dx", xd.grad, xr.grad)]
    pairs += [(k, prm.grad, P[k].grad) for k, prm in tf.named_parameters()]
    num = den = 0.0
    worst = ("", 0.0)
    for name, got, ref in pairs[2:]:
        assert got is not None, name
        d = got.double().cpu() - ref
        num += float(d.square().sum())
        den += float(ref.square().sum())
        e = _rel(got, ref)[0]
        if e > worst[1]:
            worst = (name, e)
    l2 = (num / den) ** 0.5
    ey, ex = _rel(*pairs[0][1:]), _rel(*pairs[1][1:])
    print(f"\n[dropout] {case} {mode}: y {ey}, dx {ex}, worst grad {worst}, grad rel-L2 {l2:.2e}")
    if mode == "fp32":
        assert ey[0] <= 1e-4 and ex[0] <= 1e-4, (ey, ex)
        assert worst[1] <= 1e-4 and l2 <= 1e-5, (worst, l2)
    else:
        assert ey[1] <= 8e-3 and ex[1] <= 8e-3, (ey, ex)
        assert l2 <= 8e-3, (worst, l2)


_KW = dict(image_size=32, tactile_size=16, image_patch_size=8, tactile_patch_size=4, dim=128, depth=3, heads=2, mlp_dim=256)
_MKW = dict(decoder_dim=128, masking_ratio=0.75, decoder_depth=2, decoder_heads=2)


def _inputs(B=6, nt=2):
    g = torch.Generator(device="cpu").manual_seed(11)
    x = {"image": torch.rand(B, 3, 32, 32, generator=g).to(DEV)}
    for i in range(nt):
        x[f"tactile{i + 1}"] = torch.rand(B, 3, 16, 16, generator=g).to(DEV)
    noises = [torch.rand(B, 16, generator=g).to(DEV) for _ in range(1 + nt)]
    return x, noises


def _mae_run(dt, fused, chunk=None, model_seed=2, step_seed=4, p=P_DROP, eval_mode=False, **mkw):
    torch.manual_seed(model_seed)
    mae = VTMAE(encoder=VTT(dropout=p, **_KW), compute_dtype=dt, **dict(_MKW, **mkw)).to(DEV)
    if eval_mode:
        mae.eval()
    x, noises = _inputs()
    keep = (Fn.FUSED_STEP, Fn.BWD_CHUNK_LAYERS)
    Fn.FUSED_STEP, Fn.BWD_CHUNK_LAYERS = fused, chunk
    try:
        torch.manual_seed(step_seed)
        loss = mae(x, mask_noise=noises)
        assert (type(loss.grad_fn).__name__ == "MaeStepFnBackward") == (fused and chunk is None)
        (loss * 1.5).backward()
        torch.cuda.synchronize()
    finally:
        Fn.FUSED_STEP, Fn.BWD_CHUNK_LAYERS = keep
    return mae, loss.detach().cpu(), {k: v.grad.detach().cpu() for k, v in mae.named_parameters() if v.grad is not None}


def _same(a, b):
    assert torch.equal(a[1], b[1]), (a[1], b[1])
    assert a[2].keys() == b[2].keys()
    for k in a[2]:
        assert torch.equal(a[2][k], b[2][k]), k


@pytest.mark.parametrize("dt", ["fp32", "bf16"])
def test_fused_step_bit_identical_to_module_chain_with_dropout(dt):
    fused = _mae_run(dt, True)
    assert fused[0].encoder.transformer.last_dropout_seed is not None and fused[0].decoder.last_dropout_seed is None
    for chunk in (None, 1, 2):
        _same(fused, _mae_run(dt, False, chunk))


@pytest.mark.parametrize("dt", ["fp32", "bf16"])
def test_early_conv_default_architecture_runs_with_dropout(dt):
    a = _mae_run(dt, True, early_conv_masking=True)
    b = _mae_run(dt, False, early_conv_masking=True)
    _same(a, b)
    assert torch.isfinite(a[1]) and all(torch.isfinite(v).all() for v in a[2].values())


def test_seed_determinism_and_eval_identity():
    a, b = _mae_run("bf16", True), _mae_run("bf16", True)
    _same(a, b)
    c = _mae_run("bf16", True, step_seed=5)
    assert not torch.equal(a[1], c[1])
    d = _mae_run("bf16", True, p=0.0)
    assert not torch.equal(a[1], d[1])             # dropout changes the training loss
    e, f = _mae_run("bf16", True, eval_mode=True), _mae_run("bf16", True, p=0.0, eval_mode=True)
    _same(e, f)                                    # eval: bit-identical to dropout = 0 on the default kernels


@pytest.mark.parametrize("dt", ["fp32", "bf16"])
def test_extractor_with_dropout_matches_module_chain(dt):
    """MAEExtractor's chain (get_embeddings(eval=False) -> head -> token mean) as one library call against the per-module chain, with the
    MAE encoder dropping and the head not.  Same bounds as test_parity_gpu's extractor test: the token mean is a kernel in the fused call
    and torch.mean in the module chain (different summation order), so the two agree to the last bits, not bit for bit."""
    from m3l_amd.fusion import pooled_embeddings

    def run(fused, p=P_DROP):
        torch.manual_seed(2)
        mae = VTMAE(encoder=VTT(dropout=p, **_KW), compute_dtype=dt, **_MKW).to(DEV)
        head = Transformer(128, 1, 2, 64, 256).to(DEV)
        head.compute_dtype = dt
        x, _ = _inputs()
        keep = Fn.FUSED_EXTRACTOR
        Fn.FUSED_EXTRACTOR = fused
        try:
            torch.manual_seed(7)
            out = pooled_embeddings(mae, head, x)
            out.square().sum().backward()
            torch.cuda.synchronize()
        finally:
            Fn.FUSED_EXTRACTOR = keep
        grads = {k: v.grad.detach().cpu() for k, v in list(mae.named_parameters()) + [("head." + k, v) for k, v in head.named_parameters()]
                 if v.grad is not None}
        return mae, out.detach().cpu(), grads, head

    a, b = run(True), run(False)
    assert a[0].encoder.transformer.last_dropout_seed is not None and a[3].last_dropout_seed is None
    assert a[0].encoder.transformer.last_dropout_seed == b[0].encoder.transformer.last_dropout_seed
    assert float((a[1] - b[1]).abs().max()) <= 1e-6 * float(a[1].abs().max()) + 1e-7
    tol = 1e-5 if dt == "fp32" else 2e-2
    assert a[2].keys() == b[2].keys()
    for k in a[2]:
        scale = float(a[2][k].abs().max()) + 1e-12
        assert float((a[2][k] - b[2][k]).abs().max()) <= tol * scale, (k, float((a[2][k] - b[2][k]).abs().max()), scale)
    assert float((a[1] - run(True, p=0.0)[1]).abs().max()) > 1e-3 * float(a[1].abs().max())     # the encoder did drop
    # get_embeddings(eval=True) is deterministic (no dropout in eval mode)
    x, _ = _inputs()
    e1 = a[0].get_embeddings(x, eval=True).detach()
    e2 = a[0].get_embeddings(x, eval=True).detach()
    assert torch.equal(e1, e2)
