"""Attention heads 32 and 128 wide on the MI355X: the attention kernels at DH in {32, 64, 128} against torch, the stack against the
reference-held fixtures (tests/golden/make_golden_dim_head.py) and the CPU oracle with the kernel selection it must take (per-op chain
only), whole models at full depth, the fused step / extractor against their module chains, dropout, DinoVTT and the C ABI."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

from m3l_amd import VTMAE, VTT, DinoVTT, Transformer  # noqa: E402
from m3l_amd import _lib as L  # noqa: E402
from m3l_amd import functional as Fn  # noqa: E402
from oracle import vtmae_oracle as O  # noqa: E402
from test_dim_head_cpu import load_fixture  # noqa: E402

DEV = "cuda:0"
BF16_GTOL, BF16_L2TOL = 0.03, 6e-3          # tests/test_fulldepth_gpu.py
FUSED_CLASSES = ("attn_block_", "mlp_block_", "attn_t192_", "attn_tail_mlp_t192_fwd", "mlp_t192_", "qkv_bwd_t192", "enc_fwd_mega",
                 "enc_bwd_mega")


def _s():
    return torch.cuda.current_stream().cuda_stream


def _t(code):
    return torch.bfloat16 if code else torch.float32


def _tol(code):
    return dict(rtol=2e-2, atol=2e-2) if code else dict(rtol=2e-4, atol=2e-4)


def _relmax(a, ref):
    return float((a - ref).abs().max()) / max(1e-7, float(ref.abs().max()))


class _Prof:
    """kernel classes launched inside the scope (in-library profiler, as tests/test_fulldepth_gpu.py reads it)"""

    def __enter__(self):
        L.lib().m3l_prof_begin(None, 1)
        return self

    def __exit__(self, *a):
        lib = L.lib()
        lib.m3l_prof_end()
        self.kinds = set()
        for i in range(lib.m3l_prof_count()):
            name = C.create_string_buffer(96)
            a_, b, c_, d = C.c_double(), C.c_long(), C.c_double(), C.c_double()
            lib.m3l_prof_get(i, name, 96, C.byref(a_), C.byref(b), C.byref(c_), C.byref(d))
            if b.value:
                self.kinds.add(name.value.decode())

    def fused(self):
        return sorted(k for k in self.kinds if k.startswith(FUSED_CLASSES))

    def has(self, prefix):
        return any(k.startswith(prefix) for k in self.kinds)


class _Residual:
    def __init__(self, on):
        self.on = on

    def __enter__(self):
        self.old = L.lib().m3l_set_residual_bf16(self.on)

    def __exit__(self, *a):
        L.lib().m3l_set_residual_bf16(self.old)


# ---- 0. the attention kernels against torch
def _attn_ref(qkv, B, n, H, DH):
    q, k, v = [t.reshape(B, n, H, DH).transpose(1, 2) for t in qkv.float().reshape(B, n, 3 * H * DH).chunk(3, dim=-1)]
    dots = (q @ k.transpose(-1, -2)) * (DH ** -0.5)
    o = (dots.softmax(-1) @ v).transpose(1, 2).reshape(B * n, H * DH)
    return o, torch.logsumexp(dots, -1)


@pytest.mark.parametrize("DH", [32, 128])
@pytest.mark.parametrize("code", [0, 1])
@pytest.mark.parametrize("B,n,H", [(2, 48, 3), (3, 16, 1), (2, 10, 4), (2, 75, 2), (1, 192, 3), (1, 113, 6), (1, 452, 1)])
def test_attention_dh_fwd_bwd(DH, code, B, n, H):
    torch.manual_seed(n * 7 + H + DH)
    qkv = torch.randn(B * n, 3 * H * DH, device=DEV).to(_t(code))
    dO = torch.randn(B * n, H * DH, device=DEV).to(_t(code))
    o = torch.zeros(B * n, H * DH, device=DEV, dtype=_t(code))
    lse = torch.zeros(B, H, n, device=DEV)
    L.check(L.lib().m3l_op_attn_fwd_dh(code, L.ptr(qkv), L.ptr(o), L.ptr(lse), B, n, H, _s(), DH), "attn_fwd_dh")
    ref_in = qkv.float().clone().requires_grad_(True)
    ref_o, ref_lse = _attn_ref(ref_in, B, n, H, DH)
    torch.testing.assert_close(o.float(), ref_o, **_tol(code))
    torch.testing.assert_close(lse, ref_lse, rtol=1e-4, atol=2e-2 if code else 1e-4)
    dsum = torch.zeros(B, H, n, device=DEV)
    dqkv = torch.full_like(qkv, float("nan"))
    L.check(L.lib().m3l_op_attn_bwd_dh(code, L.ptr(qkv), L.ptr(o), L.ptr(dO), L.ptr(lse), L.ptr(dsum), L.ptr(dqkv), B, n, H, _s(), DH),
            "attn_bwd_dh")
    (ref_o * dO.float()).sum().backward()
    scale = ref_in.grad.abs().max().item()
    assert (dqkv.float() - ref_in.grad).abs().max().item() <= (4e-2 if code else 2e-4) * scale + 1e-5


@pytest.mark.parametrize("DH", [32, 128])
def test_attention_dh_softmax_spike(DH):
    """one key dominating from a late tile: the online-softmax rescale branch at the other head widths"""
    B, n, H = 1, 96, 1
    torch.manual_seed(3)
    qkv = 0.1 * torch.randn(B * n, 3 * DH, device=DEV)
    qkv[5, 0:DH] = 4.0
    qkv[80, DH:2 * DH] = 4.0
    o = torch.zeros(B * n, DH, device=DEV)
    lse = torch.zeros(B, H, n, device=DEV)
    L.check(L.lib().m3l_op_attn_fwd_dh(0, L.ptr(qkv), L.ptr(o), L.ptr(lse), B, n, H, _s(), DH), "attn_fwd_dh")
    ref_o, ref_lse = _attn_ref(qkv, B, n, H, DH)
    torch.testing.assert_close(o, ref_o, rtol=1e-4, atol=1e-5)
    torch.testing.assert_close(lse, ref_lse, rtol=1e-5, atol=1e-4)


@pytest.mark.parametrize("code", [0, 1])
@pytest.mark.parametrize("B,n,H", [(2, 48, 3), (1, 452, 2)])
def test_attention_dh64_is_the_64_entry_point(code, B, n, H):
    torch.manual_seed(n + H)
    qkv = torch.randn(B * n, 3 * H * 64, device=DEV).to(_t(code))
    dO = torch.randn(B * n, H * 64, device=DEV).to(_t(code))
    outs = []
    for dh in (None, 64):
        o = torch.zeros(B * n, H * 64, device=DEV, dtype=_t(code))
        lse, dsum = torch.zeros(B, H, n, device=DEV), torch.zeros(B, H, n, device=DEV)
        dqkv = torch.zeros_like(qkv)
        if dh is None:
            L.check(L.lib().m3l_op_attn_fwd(code, L.ptr(qkv), L.ptr(o), L.ptr(lse), B, n, H, _s()), "attn_fwd")
            L.check(L.lib().m3l_op_attn_bwd(code, L.ptr(qkv), L.ptr(o), L.ptr(dO), L.ptr(lse), L.ptr(dsum), L.ptr(dqkv), B, n, H, _s()), "attn_bwd")
        else:
            L.check(L.lib().m3l_op_attn_fwd_dh(code, L.ptr(qkv), L.ptr(o), L.ptr(lse), B, n, H, _s(), dh), "attn_fwd_dh")
            L.check(L.lib().m3l_op_attn_bwd_dh(code, L.ptr(qkv), L.ptr(o), L.ptr(dO), L.ptr(lse), L.ptr(dsum), L.ptr(dqkv), B, n, H, _s(), dh),
                    "attn_bwd_dh")
        torch.cuda.synchronize()
        outs.append((o, lse, dsum, dqkv))
    for a, b in zip(*outs):
        assert torch.equal(a, b)


# ---- 1. the reference-held fixtures
@pytest.mark.parametrize("name", ["block_stack_dh32", "block_stack_dh128"])
@pytest.mark.parametrize("n", [48, 192])
@pytest.mark.parametrize("dt,rb", [("fp32", 0), ("bf16", 0), ("bf16", 1)])
def test_stack_vs_reference_held_block_dim_head(name, n, dt, rb):
    """bounds of tests/test_block_fixture_gpu.py on block_stack.npz (fp32 1e-5; bf16 per residual mode)"""
    meta, params, data, z = load_fixture(name)
    D, depth, heads, mlp, dh = meta["D"], meta["depth"], meta["heads"], meta["mlp"], meta["dim_head"]
    tf = Transformer(D, depth, heads, dh, mlp)
    tf.load_state_dict({k: torch.tensor(v) for k, v in params.items()}, strict=True)
    tf.compute_dtype = dt
    tf = tf.to(DEV)
    x, cot = torch.tensor(data[n][0]).to(DEV).requires_grad_(True), torch.tensor(data[n][1]).to(DEV)
    with _Residual(rb), _Prof() as prof:
        y = tf(x)
        (y * cot).sum().backward()
        torch.cuda.synchronize()
    assert prof.has("attn_fwd[") and prof.has("attn_bwd[") and not prof.fused(), prof.fused()
    ytol, gtol = (1e-5, 1e-5) if dt == "fp32" else (1e-2, 2e-2)
    ey = _relmax(y.detach().cpu(), torch.tensor(z[f"n{n}/y"]))
    edx = _relmax(x.grad.cpu(), torch.tensor(z[f"n{n}/dx"]))
    worst = ("", 0.0)
    for k, p in tf.named_parameters():
        g = p.grad.cpu()
        if g.dim() == 2:
            g = g[torch.tensor(z["rows/" + k])]
        e = _relmax(g, torch.tensor(z[f"n{n}/grad/" + k]))
        worst = max(worst, (k, e), key=lambda t: t[1])
    print(f"\n[{name}] n={n} {dt} rb {rb}: y {ey:.2e} dx {edx:.2e} worst grad {worst[0]} {worst[1]:.2e}")
    assert ey <= ytol and edx <= gtol and worst[1] <= gtol, (ey, edx, worst)


# ---- 2. the stack against oracle.transformer, and the kernels it takes
def _stack_check(D, heads, dh, n, dt, B=3, mlp=None):
    mlp = mlp or 2 * D
    torch.manual_seed(D + heads + dh + n)
    tf = Transformer(D, 2, heads, dh, mlp)
    g = torch.Generator().manual_seed(n)
    with torch.no_grad():
        for p in tf.parameters():
            if p.dim() == 1:
                p.add_(0.1 * torch.randn(p.shape, generator=g))
    tf.compute_dtype = dt
    tf = tf.to(DEV)
    x = (torch.randn(B, n, D, generator=g) * 1.5)
    cot = torch.randn(B, n, D, generator=g)
    P = {"t." + k: v.detach().cpu().clone().requires_grad_(True) for k, v in tf.state_dict().items()}
    xo = x.clone().requires_grad_(True)
    yo = O.transformer(xo, P, "t.", 2, heads, dh)
    (yo * cot).sum().backward()
    xg = x.to(DEV).requires_grad_(True)
    with _Prof() as prof:
        y = tf(xg)
        (y * cot.to(DEV)).sum().backward()
        torch.cuda.synchronize()
    ytol, gtol = (1e-4, 1e-4) if dt == "fp32" else (1e-2, 3e-2)
    ey, edx = _relmax(y.detach().cpu(), yo.detach()), _relmax(xg.grad.cpu(), xo.grad)
    worst = max(((k, _relmax(p.grad.cpu(), P["t." + k].grad)) for k, p in tf.named_parameters()), key=lambda t: t[1])
    print(f"\n[dim_head stack] D {D} heads {heads} dh {dh} n {n} {dt}: y {ey:.2e} dx {edx:.2e} worst {worst[0]} {worst[1]:.2e}")
    assert ey <= ytol and edx <= gtol and worst[1] <= gtol, (ey, edx, worst)
    return prof


@pytest.mark.parametrize("D,heads,dh", [(192, 6, 32), (192, 3, 32), (256, 4, 128), (128, 1, 128)])
@pytest.mark.parametrize("n", [1, 48, 192, 260])
@pytest.mark.parametrize("dt", ["fp32", "bf16"])
def test_stack_dim_head_vs_oracle_on_per_op_chain(D, heads, dh, n, dt):
    """B = 128 at n = 192: the batch at which the row-tile kernels would take D = 192 / 3 heads and D = 256 / 4 heads at 64-wide heads"""
    prof = _stack_check(D, heads, dh, n, dt, B=128 if n == 192 else 3)
    assert prof.has("attn_fwd[") and prof.has("attn_bwd["), sorted(prof.kinds)
    assert not prof.fused(), prof.fused()


@pytest.mark.parametrize("D,heads,n,B", [(192, 3, 48, 3), (256, 4, 192, 128)])
def test_dim_head_64_still_takes_fused_kernels(D, heads, n, B):
    """the gate is not always closed: the same shapes at dim_head = 64 take the block (n <= 48) / row-tile (n <= 192) kernels"""
    prof = _stack_check(D, heads, 64, n, "bf16", B=B)
    assert prof.fused(), sorted(prof.kinds)


# ---- 3. whole model at full depth
CFG2_ENC = dict(image_size=64, tactile_size=32, image_patch_size=8, tactile_patch_size=4, dim=192, depth=12, heads=6, mlp_dim=768, dim_head=32)
CFG2_MAE = dict(decoder_dim=192, masking_ratio=0.75, decoder_depth=4, decoder_heads=3, decoder_dim_head=128)
CFG2_O = O.OracleCfg(64, 32, 8, 4, 192, 12, 6, 768, 3, 2, 192, 4, 3, 0.75, dim_head=32, dec_dim_head=128)


def _data(ocfg, B, seed, C=3, hw=(64, 32), k=2):
    g = torch.Generator(device="cpu").manual_seed(seed)
    x = {"image": torch.rand(B, C, hw[0], hw[0], generator=g)}
    for i in range(k):
        x[f"tactile{i + 1}"] = torch.rand(B, C, hw[1], hw[1], generator=g)
    noises = [torch.rand(B, ocfg.n_img, generator=g)] + [torch.rand(B, ocfg.n_tac, generator=g) for _ in range(k)]
    return x, noises


def _perturb(mae):
    g = torch.Generator(device="cpu").manual_seed(99)
    with torch.no_grad():
        for p in mae.parameters():
            if p.dim() == 1:
                p.add_((0.05 * torch.randn(p.shape, generator=g)).to(p.device))


@pytest.mark.parametrize("dt,ltol,gtol,l2tol", [("fp32", 1e-4, 2e-3, 1e-4), ("bf16", 1e-2, BF16_GTOL, BF16_L2TOL)])
def test_cfg2_full_depth_dim_head_vs_oracle(dt, ltol, gtol, l2tol):
    torch.manual_seed(0)
    mae = VTMAE(encoder=VTT(**CFG2_ENC), compute_dtype=dt, **CFG2_MAE).to(DEV)
    _perturb(mae)
    x, noises = _data(CFG2_O, 16, seed=1)
    loss = mae({k: v.to(DEV) for k, v in x.items()}, mask_noise=[n.to(DEV) for n in noises])
    loss.backward()
    torch.cuda.synchronize()
    P = {k: v.detach().cpu().clone().requires_grad_(v.dtype.is_floating_point) for k, v in mae.state_dict().items()}
    r = O.vtmae_forward(P, CFG2_O, x, noises)
    r["loss"].backward()
    assert torch.equal(mae.last_mask[0].cpu(), r["masked_indices"]) and torch.equal(mae.last_mask[1].cpu(), r["unmasked_indices"])
    rel = abs(float(loss.detach()) - float(r["loss"])) / abs(float(r["loss"]))
    num = den = 0.0
    worst = ("", 0.0)
    for name, p in mae.named_parameters():
        ref = P[name].grad
        if ref is None:
            assert p.grad is None, name
            continue
        d = p.grad.cpu() - ref
        e = float(d.abs().max()) / max(1e-7, float(ref.abs().max()))
        worst = max(worst, (name, e), key=lambda t: t[1])
        num += float(d.double().square().sum())
        den += float(ref.double().square().sum())
    l2 = (num / den) ** 0.5
    print(f"\n[dim_head cfg2] {dt}: loss rel {rel:.2e}, worst grad {worst[0]} {worst[1]:.2e}, rel-L2 {l2:.2e}")
    assert rel <= ltol and worst[1] <= gtol and l2 <= l2tol, (rel, worst, l2)


# ---- 4. fused step against the module chain
@pytest.mark.parametrize("arch", ["cfg2_bf16", "cfg2_fp32", "m3l_default_bf16"])
def test_fused_step_dim_head_is_bit_identical_to_module_chain(arch):
    if arch.startswith("cfg2"):
        kw = dict(image_size=64, tactile_size=32, image_patch_size=8, tactile_patch_size=4, dim=192, depth=2, heads=6, mlp_dim=768, dim_head=32)
        mkw = dict(decoder_dim=192, masking_ratio=0.75, decoder_depth=2, decoder_heads=6, decoder_dim_head=32)
        C_, hw, B = 3, (64, 32), 6
    else:      # M3L's default architecture: 256 / 4 / 4 heads, EarlyCNN front end; dim_head 32 -> inner width 128 != 256
        kw = dict(image_size=64, tactile_size=32, image_patch_size=8, tactile_patch_size=4, dim=256, depth=4, heads=4, mlp_dim=512, dim_head=32,
                  image_channels=12, tactile_channels=12, num_tactiles=2, frame_stack=4)
        mkw = dict(decoder_dim=256, masking_ratio=0.95, decoder_depth=3, decoder_heads=4, decoder_dim_head=32, num_tactiles=2,
                   early_conv_masking=True, frame_stack=4)
        C_, hw, B = 12, (64, 32), 4
    dt = "fp32" if arch.endswith("fp32") else "bf16"
    g = torch.Generator(device="cpu").manual_seed(11)
    x = {"image": torch.rand(B, C_, hw[0], hw[0], generator=g).to(DEV)}
    for i in range(2):
        x[f"tactile{i + 1}"] = torch.rand(B, C_, hw[1], hw[1], generator=g).to(DEV)
    n_img, n_tac = (hw[0] // 8) ** 2, (hw[1] // 4) ** 2
    noises = [torch.rand(B, n_img, generator=g).to(DEV)] + [torch.rand(B, n_tac, generator=g).to(DEV) for _ in range(2)]

    def run(fused):
        torch.manual_seed(2)
        mae = VTMAE(encoder=VTT(**kw), compute_dtype=dt, **mkw).to(DEV)
        keep = Fn.FUSED_STEP
        Fn.FUSED_STEP = fused
        try:
            loss = mae(x, mask_noise=noises)
            assert (type(loss.grad_fn).__name__ == "MaeStepFnBackward") == fused
            (loss * 1.5).backward()
        finally:
            Fn.FUSED_STEP = keep
        torch.cuda.synchronize()
        return loss.detach().clone(), mae.last_mask, {n: (None if p.grad is None else p.grad.clone()) for n, p in mae.named_parameters()}

    l0, m0, g0 = run(False)
    l1, m1, g1 = run(True)
    assert torch.equal(l0, l1) and torch.equal(m0[0], m1[0]) and torch.equal(m0[1], m1[1])
    for n in g0:
        assert (g0[n] is None) == (g1[n] is None), n
        if g0[n] is not None and n in ("encoder.pos_embedding", "decoder_pos_emb.weight"):
            assert float((g0[n] - g1[n]).abs().max()) <= 1e-5 * float(g0[n].abs().max()) + 1e-9, n
        elif g0[n] is not None:
            assert torch.equal(g0[n], g1[n]), n


# ---- 5. extractor
@pytest.mark.parametrize("dt", ["fp32", "bf16"])
def test_extractor_dim_head_vs_oracle_and_chain(dt):
    """fusion.pooled_embeddings (MAEExtractor.forward's chain: get_embeddings -> 1-layer Transformer -> token mean) over an encoder and a
    head with dim_head = 32: m3l_extractor_fwd / _bwd against the per-module Functions, and against the oracle"""
    from m3l_amd.fusion import pooled_embeddings
    kw = dict(image_size=32, tactile_size=16, image_patch_size=8, tactile_patch_size=4, dim=128, depth=2, heads=4, mlp_dim=256, dim_head=32)
    B = 3
    g = torch.Generator(device="cpu").manual_seed(4)
    x = {"image": torch.rand(B, 3, 32, 32, generator=g), "tactile1": torch.rand(B, 3, 16, 16, generator=g),
         "tactile2": torch.rand(B, 3, 16, 16, generator=g)}

    def run(fused):
        torch.manual_seed(5)
        mae = VTMAE(encoder=VTT(**kw), decoder_dim=128, decoder_depth=1, decoder_heads=2, compute_dtype=dt).to(DEV)
        head = Transformer(128, 1, 4, 32, 256)
        head.compute_dtype = dt
        head = head.to(DEV)
        keep = Fn.FUSED_EXTRACTOR
        Fn.FUSED_EXTRACTOR = fused
        try:
            feat = pooled_embeddings(mae, head, {k: v.to(DEV) for k, v in x.items()})
            feat.square().sum().backward()
        finally:
            Fn.FUSED_EXTRACTOR = keep
        torch.cuda.synchronize()
        grads = {"mae." + n: p.grad.clone() for n, p in mae.named_parameters() if p.grad is not None}
        grads.update({"head." + n: p.grad.clone() for n, p in head.named_parameters()})
        return feat.detach().clone(), grads, mae, head

    f0, g0, mae, head = run(False)
    f1, g1, _, _ = run(True)
    # bounds of test_parity_gpu.py::test_fused_extractor_is_bit_identical_to_module_chain: the same kernels up to the token mean (the
    # library sums the tokens in order, torch.mean in its own order)
    assert float((f0 - f1).abs().max()) <= 1e-6 * float(f0.abs().max()) + 1e-7
    tol = 1e-5 if dt == "fp32" else 2e-2
    assert set(g0) == set(g1)
    for n in g0:
        assert float((g0[n] - g1[n]).abs().max()) <= tol * (float(g0[n].abs().max()) + 1e-12), n
    cfg = O.OracleCfg(32, 16, 8, 4, 128, 2, 4, 256, 3, 2, 128, 1, 2, 0.75, dim_head=32)
    P = {k: v.detach().cpu().clone().requires_grad_(v.dtype.is_floating_point) for k, v in mae.state_dict().items()}
    PH = {"t." + k: v.detach().cpu().clone().requires_grad_(True) for k, v in head.state_dict().items()}
    ref = O.transformer(O.get_embeddings(P, cfg, x), PH, "t.", 1, 4, 32).mean(dim=1)
    ref.square().sum().backward()
    ftol, gtol = (1e-4, 1e-3) if dt == "fp32" else (2e-2, 3e-2)
    assert _relmax(f1.cpu(), ref.detach()) <= ftol
    for name in ("encoder.transformer.layers.0.0.to_qkv.weight", "encoder.transformer.layers.1.0.to_out.0.weight"):
        assert _relmax(g1["mae." + name].cpu(), P[name].grad) <= gtol, name
    assert _relmax(g1["head.layers.0.0.to_qkv.weight"].cpu(), PH["t.layers.0.0.to_qkv.weight"].grad) <= gtol


# ---- 6. dropout together with dim_head
def test_dropout_with_dim_head_vs_oracle(monkeypatch):
    import test_dropout_oracle_gpu as TD
    enc = dict(image_size=64, tactile_size=32, image_patch_size=8, tactile_patch_size=4, dim=192, depth=4, heads=6, mlp_dim=768, dim_head=32)
    mae = dict(decoder_dim=192, masking_ratio=0.75, decoder_depth=2, decoder_heads=3)
    ocfg = O.OracleCfg(64, 32, 8, 4, 192, 4, 6, 768, 3, 2, 192, 2, 3, 0.75, dim_head=32)
    TD._run(monkeypatch, enc, mae, ocfg, 16, 3, (64, 32), 2, "bf16", 1e-2, BF16_GTOL, BF16_L2TOL)


# ---- 7. DinoVTT
@pytest.mark.parametrize("dt", ["fp32", "bf16"])
def test_dino_vtt_dim_head_vs_oracle(dt):
    torch.manual_seed(8)
    enc = DinoVTT(image_size=32, tactile_size=32, image_patch_size=8, tactile_patch_size=8, dim=192, depth=2, heads=6, mlp_dim=384,
                  num_tactiles=2, dim_head=32, compute_dtype=dt).to(DEV)
    _perturb(enc)
    g = torch.Generator(device="cpu").manual_seed(9)
    x = {k: torch.rand(2, 3, 32, 32, generator=g) for k in ("image", "tactile1", "tactile2")}
    out = enc({k: v.to(DEV) for k, v in x.items()})
    out.square().mean().backward()
    torch.cuda.synchronize()
    P = {k: v.detach().cpu().clone().requires_grad_(v.dtype.is_floating_point) for k, v in enc.state_dict().items()}
    r = O.vtt_dino_forward(P, image_patch=8, tactile_patch=8, depth=2, heads=6, x=x, dim_head=32)
    r["x_norm_patchtokens"].square().mean().backward()
    otol, gtol = (1e-4, 5e-3) if dt == "fp32" else (3e-2, 3e-2)
    assert _relmax(out.detach().cpu(), r["x_norm_patchtokens"].detach()) <= otol
    for name, prm in enc.named_parameters():
        ref = P[name].grad
        if ref is None:
            assert prm.grad is None, name
            continue
        assert _relmax(prm.grad.cpu(), ref) <= gtol, name


# ---- 8. C ABI
def _tf_call(cfg, B, n, tensors, x):
    lib = L.lib()
    nb = lib.m3l_transformer_ws_bytes(C.byref(cfg), B, n)
    assert nb > 0
    ws = torch.zeros(nb, dtype=torch.uint8, device=DEV)
    y_t = torch.zeros(B * n * cfg.dim, dtype=torch.bfloat16 if cfg.dtype else torch.float32, device=DEV)
    y32 = torch.zeros(B * n, cfg.dim, device=DEV)
    L.check(lib.m3l_transformer_fwd(C.byref(cfg), B, n, L.ptr(x), L.ptr_array(tensors), L.ptr(ws), L.ptr(y_t), L.ptr(y32), _s()),
            "transformer_fwd")
    torch.cuda.synchronize()
    return y32


@pytest.mark.parametrize("dt", [0, 1])
def test_c_abi_dim_head_zero_means_64_and_48_is_refused(dt):
    torch.manual_seed(1)
    tf = Transformer(192, 2, 3, 64, 384).to(DEV)
    B, n = 2, 40
    x = torch.randn(B * n, 192, device=DEV)
    tensors = tf._tensors()
    y0 = _tf_call(L.TfCfg(192, 2, 3, 384, 1, dt, 0), B, n, tensors, x)
    y64 = _tf_call(L.TfCfg(192, 2, 3, 384, 1, dt, 64), B, n, tensors, x)
    assert torch.equal(y0, y64)
    lib = L.lib()
    bad = L.TfCfg(192, 2, 3, 384, 1, dt, 48)
    assert lib.m3l_transformer_ws_bytes(C.byref(bad), B, n) == 0
    ws = torch.zeros(1 << 20, dtype=torch.uint8, device=DEV)
    y32 = torch.zeros(B * n, 192, device=DEV)
    rc = lib.m3l_transformer_fwd(C.byref(bad), B, n, L.ptr(x), L.ptr_array(tensors), L.ptr(ws), None, L.ptr(y32), _s())
    assert rc != 0
    buf = C.create_string_buffer(512)
    lib.m3l_last_error(buf, 512)
    assert b"dim_head" in buf.value, buf.value
