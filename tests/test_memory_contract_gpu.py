"""The memory contract of include/m3l_amd.h on a real MI355X: every entry point stays inside the workspace and the outputs it was handed
and computes the same bits whatever they held before.

Each case runs one seeded workload three times — as the rest of the suite runs it, then twice under tests/memguard.py, which hands every
float32 / bf16 / uint8 allocation m3l_amd makes (workspaces through `functional._ws`, outputs through torch.empty / empty_like) out of a
larger block [guard | payload | guard] pre-filled with 0xFF (NaN) and with 0x00 — and asserts
  (a) every output, the loss, the index lists and every gradient bit-identical (torch.equal) across the three runs,
  (b) all of them finite,
  (c) every guard byte untouched after the forward and again after the backward (after a device synchronise: weight gradients run on the
      library's side stream),
  (d) that workspaces and tensors really went through the guard, and that every workspace had the size its *_ws_bytes function returned.
No tolerance appears in this file: the library has no float atomics and fixes its reduction orders; values are held to the oracle by the
other files.  Kernel families are chosen through the m3l_set_* switches at the shapes test_block_fixture_gpu.py found to change code path
(ragged last row tile, tiles that straddle samples, partial 16-row tile, one / two key tiles, n = 1, the two-block MLP ring).

The last tests pin two things the header now states: which gradient slots m3l_mae_step_bwd overwrites in direct-gradient mode (the flat
buffer starts as NaN), and that a flat parameter / gradient buffer whose members are only 4-byte aligned (patch dims 147 / 75) computes
what the per-tensor path computes."""
import contextlib
import ctypes as C
import os
from functools import partial

import numpy as np
import pytest
import torch

import memguard as MG

pytestmark = pytest.mark.gpu

import m3l_amd  # noqa: E402
from m3l_amd import VTMAE, VTT, Transformer  # noqa: E402
from m3l_amd import _lib as L  # noqa: E402
from m3l_amd import functional as Fn  # noqa: E402

DEV = "cuda:0"


def _s():
    return torch.cuda.current_stream().cuda_stream


def _t(code):
    return torch.bfloat16 if code else torch.float32


@contextlib.contextmanager
def _switches(**kw):
    """m3l_set_<name>(value) for the duration of a case: attn_block, t192, t192_tt, enc_mega, residual_bf16, rowln, direct_conv."""
    lib, old = L.lib(), []
    try:
        for k, v in kw.items():
            old.append((k, getattr(lib, "m3l_set_" + k)(v)))
        yield
    finally:
        for k, v in reversed(old):
            getattr(lib, "m3l_set_" + k)(v)


def _grads(module):
    return {n: p.grad for n, p in module.named_parameters() if p.grad is not None}


# ---------------------------------------------------------------------------------------------------------------- transformer stack
def _stack(D, depth, heads, mlp, n, B, dt, dim_head=64, dropout=0.0):
    torch.manual_seed(D + n + B)
    tf = Transformer(D, depth, heads, dim_head, mlp, dropout)
    g = torch.Generator().manual_seed(n)
    with torch.no_grad():
        for p in tf.parameters():
            if p.dim() == 1:
                p.add_(0.1 * torch.randn(p.shape, generator=g))
    tf.compute_dtype = dt
    tf = tf.to(DEV)
    x = (torch.randn(B, n, D, generator=g) * 1.5).to(DEV)
    cot = torch.randn(B, n, D, generator=g).to(DEV)
    return tf, x, cot


def _stack_work(tf, x, cot):
    def work(g):
        torch.manual_seed(17)                       # (a stack with dropout draws its mask seed from torch's CPU generator)
        tf.zero_grad(set_to_none=True)
        xg = x.clone().requires_grad_(True)
        y = tf(xg)
        g.check("after the forward")
        (y * cot).sum().backward()
        g.check("after the backward")
        return {"y": y, "dx": xg.grad, "grad": _grads(tf)}
    return work


def _stack_contract(monkeypatch, shape, dt, depth=2, dim_head=64, dropout=0.0, **sw):
    D, heads, mlp, n, B = shape
    tf, x, cot = _stack(D, depth, heads, mlp, n, B, dt, dim_head, dropout)
    with _switches(**sw):
        counts = MG.run_contract(monkeypatch, _stack_work(tf, x, cot))
    assert all(c == counts[0] for c in counts)


EDGE = [(192, 3, 768, 20, 5), (128, 2, 64, 33, 3), (192, 3, 384, 1, 7), (192, 3, 768, 48, 7)]
# per shape: the three block modes in bf16 on the fp32 residual stream, the bf16 residual stream where it engages (both halves of every
# layer block kernels: mode 3), and fp32 compute
EDGE_RUNS = [("bf16", 0, 0), ("bf16", 1, 0), ("bf16", 3, 0), ("bf16", 3, 1), ("fp32", 1, 0)]


@pytest.mark.parametrize("dt,mode,rb", EDGE_RUNS)
@pytest.mark.parametrize("shape", EDGE, ids=lambda s: "x".join(map(str, s)))
def test_block_kernels_edge_lengths(monkeypatch, shape, dt, mode, rb):
    _stack_contract(monkeypatch, shape, dt, attn_block=mode, residual_bf16=rb)


@pytest.mark.parametrize("mega,rb", [(0, 0), (3, 0), (1, 1)])
def test_one_launch_stack_depth6(monkeypatch, mega, rb):
    """enc_mega.hip at depth 6: the last backward group is shorter than the stack's layers-per-launch (bit 2 runs the fp32 residual stream)."""
    _stack_contract(monkeypatch, (192, 3, 768, 48, 7), "bf16", depth=6, attn_block=3, enc_mega=mega, residual_bf16=rb)


ROWTILE = [(192, 3, 768, 100, 3), (192, 3, 768, 192, 129), (192, 3, 768, 452, 64), (256, 4, 512, 10, 41), (384, 6, 1536, 113, 5)]
# t192 3 = the library's own tile choice, 7 = every row-tiled kernel forced at any M (small ragged shapes reach the tail handling);
# tt 6 = 96-row tall tiles (D = 192 only); residual stream bf16 (the default) and fp32
ROWTILE_CASES = [(s, t192, 12, rb) for s in ROWTILE for t192, rb in ((3, 1), (7, 0), (7, 1))] + \
                [(s, t192, 6, 1) for s in ROWTILE if s[0] == 192 for t192 in (3, 7)]


@pytest.mark.parametrize("shape,t192,tt,rb", ROWTILE_CASES, ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else str(v))
def test_row_tiled_kernels_ragged_tiles(monkeypatch, shape, t192, tt, rb):
    _stack_contract(monkeypatch, shape, "bf16", attn_block=1, t192=t192, t192_tt=tt, residual_bf16=rb)


def test_row_tile_shape_in_fp32_compute(monkeypatch):
    """The same ragged shape in fp32 compute, where the row-tile request falls back to the per-op kernels."""
    _stack_contract(monkeypatch, ROWTILE[0], "fp32", attn_block=1, t192=7)


@pytest.mark.parametrize("n", [1, 48, 260])
@pytest.mark.parametrize("D,heads,dh,dt", [(192, 6, 32, "bf16"), (192, 3, 32, "fp32"), (256, 4, 128, "bf16"), (128, 1, 128, "fp32")])
def test_dim_head_32_and_128_per_op_chain(monkeypatch, D, heads, dh, dt, n):
    _stack_contract(monkeypatch, (D, heads, 2 * D, n, 3), dt, dim_head=dh)


@pytest.mark.parametrize("dt", ["bf16", "fp32"])
@pytest.mark.parametrize("shape", [(192, 3, 768, 48, 5), (192, 3, 768, 200, 4)], ids=["short", "long"])
def test_dropout_stack(monkeypatch, shape, dt):
    D, heads, mlp, n, B = shape
    tf, x, cot = _stack(D, 2, heads, mlp, n, B, dt, dropout=0.1)
    assert tf.training
    counts = MG.run_contract(monkeypatch, _stack_work(tf, x, cot))
    assert tf.last_dropout_seed is not None and counts[0] == counts[1]


def test_chunked_backward_one_layer_groups(monkeypatch):
    """functional.BWD_CHUNK_LAYERS = 1 at cfg 5's decoder shape: a 1-layer weight-gradient group needs more slab space than a multi-layer
    one (the shape of test_chunked_backward_remainder_groups_fit_the_workspace)."""
    tf, x, cot = _stack(384, 3, 4, 1536, 75, 128, "bf16")
    monkeypatch.setattr(Fn, "BWD_CHUNK_LAYERS", 1)
    MG.run_contract(monkeypatch, _stack_work(tf, x, cot))


@pytest.mark.parametrize("dt", ["fp32", "bf16"])
def test_fused_gemm_layernorm_path(monkeypatch, dt):
    _stack_contract(monkeypatch, (192, 3, 768, 48, 5), dt, rowln=1)


# ---------------------------------------------------------------------------------------------------------------------------- MAE step
CFG2 = (dict(image_size=64, tactile_size=32, image_patch_size=8, tactile_patch_size=4, dim=192, depth=2, heads=3, mlp_dim=768),
        dict(decoder_dim=192, masking_ratio=0.75, decoder_depth=1, decoder_heads=3))


def _mae(enc_kw, mae_kw, B, dt, seed=0):
    torch.manual_seed(seed)
    mae = VTMAE(encoder=VTT(**enc_kw), compute_dtype=dt, **mae_kw).to(DEV)
    k = enc_kw.get("num_tactiles", 2)
    Ci, Ct = enc_kw.get("image_channels", 3), enc_kw.get("tactile_channels", 3)
    hi, ht = enc_kw["image_size"], enc_kw["tactile_size"]
    g = torch.Generator().manual_seed(seed + 1)
    x = {"image": torch.rand(B, Ci, hi, hi, generator=g).to(DEV)}
    for i in range(k):
        x[f"tactile{i + 1}"] = torch.rand(B, Ct, ht, ht, generator=g).to(DEV)
    n_img, n_tac = (hi // enc_kw["image_patch_size"]) ** 2, (ht // enc_kw["tactile_patch_size"]) ** 2
    noises = [torch.rand(B, n_img, generator=g).to(DEV)] + [torch.rand(B, n_tac, generator=g).to(DEV) for _ in range(k)]
    return mae, x, noises


def _mae_work(mae, x, noises, fused):
    def work(g):
        mae.zero_grad(set_to_none=True)
        keep = Fn.FUSED_STEP
        Fn.FUSED_STEP = fused
        try:
            loss = mae(x, mask_noise=noises)
            assert (type(loss.grad_fn).__name__ == "MaeStepFnBackward") == fused
            g.check("after the forward")
            loss.backward()
        finally:
            Fn.FUSED_STEP = keep
        g.check("after the backward")
        return {"loss": loss, "masked": mae.last_mask[0], "unmasked": mae.last_mask[1], "grad": _grads(mae)}
    return work


def _mae_contract(monkeypatch, enc_kw, mae_kw, B, dt, fused, **sw):
    mae, x, noises = _mae(enc_kw, mae_kw, B, dt)
    with _switches(**sw):
        MG.run_contract(monkeypatch, _mae_work(mae, x, noises, fused))
    return mae


@pytest.mark.parametrize("fused", [False, True], ids=["chain", "fused"])
@pytest.mark.parametrize("dt", ["bf16", "fp32"])
@pytest.mark.parametrize("B", [5, 41])
def test_mae_cfg2_geometry(monkeypatch, B, dt, fused):
    _mae_contract(monkeypatch, *CFG2, B=B, dt=dt, fused=fused)


def test_mae_cfg2_b256_bf16(monkeypatch):
    """144 masked rows x 256 samples: more than four rows per partial-row block, so the grid-stride loops of the masked MSE / patch
    LayerNorm backward and the capped partial-row workspaces are in play."""
    mae = _mae_contract(monkeypatch, *CFG2, B=256, dt="bf16", fused=True)
    assert mae.last_mask[0].shape == (256, 144) and 256 * 144 > 4 * 1024          # m3l_part_blocks() is 1024 unless the environment says otherwise


MAE_ARCHS = {
    # name: (encoder kw, VTMAE kw)
    "learnedpos": (dict(image_size=32, tactile_size=16, image_patch_size=8, tactile_patch_size=4, dim=128, depth=2, heads=2, mlp_dim=256),
                   dict(decoder_dim=128, decoder_depth=1, decoder_heads=2, use_sincosmod_encodings=False)),
    "vision_only": (dict(image_size=32, tactile_size=16, image_patch_size=8, tactile_patch_size=4, dim=128, depth=2, heads=2, mlp_dim=256, num_tactiles=0),
                    dict(decoder_dim=128, decoder_depth=1, decoder_heads=2, num_tactiles=0)),
    "decdim": (dict(image_size=32, tactile_size=16, image_patch_size=8, tactile_patch_size=4, dim=128, depth=2, heads=2, mlp_dim=256),
               dict(decoder_dim=64, decoder_depth=1, decoder_heads=1)),
    "pd147_75": (dict(image_size=56, tactile_size=30, image_patch_size=7, tactile_patch_size=5, dim=128, depth=1, heads=2, mlp_dim=256),
                 dict(decoder_dim=128, decoder_depth=1, decoder_heads=2)),
    "pd588": (dict(image_size=70, tactile_size=70, image_patch_size=14, tactile_patch_size=14, dim=128, depth=1, heads=2, mlp_dim=256),
              dict(decoder_dim=128, masking_ratio=0.8, decoder_depth=1, decoder_heads=2)),
    "pd2352": (dict(image_size=70, tactile_size=70, image_patch_size=14, tactile_patch_size=14, dim=128, depth=1, heads=2, mlp_dim=256,
                    image_channels=12, tactile_channels=12, frame_stack=4),
               dict(decoder_dim=128, masking_ratio=0.8, decoder_depth=1, decoder_heads=2, frame_stack=4)),
}


@pytest.mark.parametrize("dt,fused", [("bf16", True), ("fp32", False), ("bf16", False), ("fp32", True)],
                         ids=["bf16-fused", "fp32-chain", "bf16-chain", "fp32-fused"])
@pytest.mark.parametrize("arch", list(MAE_ARCHS))
def test_mae_architectures(monkeypatch, arch, dt, fused):
    _mae_contract(monkeypatch, *MAE_ARCHS[arch], B=3, dt=dt, fused=fused)


@pytest.mark.parametrize("direct", [0, 1], ids=["im2col", "direct_conv"])
@pytest.mark.parametrize("dt,fused", [("bf16", True), ("fp32", False), ("bf16", False)], ids=["bf16-fused", "fp32-chain", "bf16-chain"])
def test_mae_early_conv_frame_stack4(monkeypatch, dt, fused, direct):
    """The reference's default front end (early_conv_masking=True, frame_stack 4 -> 12 channels): EarlyCnnFn + TokensAssembleFn in the
    module chain, the same kernels inside the fused step; direct convolutions and the im2col + GEMM path."""
    enc = dict(image_size=64, tactile_size=32, image_patch_size=8, tactile_patch_size=4, dim=256, depth=2, heads=4, mlp_dim=512,
               image_channels=12, tactile_channels=12, frame_stack=4)
    kw = dict(decoder_dim=256, masking_ratio=0.95, decoder_depth=1, decoder_heads=4, early_conv_masking=True, frame_stack=4)
    _mae_contract(monkeypatch, enc, kw, B=5, dt=dt, fused=fused, direct_conv=direct)


@pytest.mark.parametrize("dt", ["fp32", "bf16"])
def test_reconstruct_with_dumps(monkeypatch, dt):
    enc_kw = dict(image_size=32, tactile_size=16, image_patch_size=8, tactile_patch_size=4, dim=64, depth=2, heads=2, mlp_dim=128)
    mae, x, noises = _mae(enc_kw, dict(decoder_dim=64, decoder_depth=1, decoder_heads=2), 3, dt)
    mae.eval()

    def work(g):
        r = dict(mae.reconstruct(x, mask_noise=noises))
        g.check("after reconstruct")
        tm = r.pop("tactile_masked")                  # masked tactile patches are +inf by definition (the reference's marker): kept as a pattern
        assert not bool(torch.isnan(tm).any())
        r["tactile_masked_marker"] = torch.isposinf(tm).to(torch.uint8)
        r["tactile_masked_visible"] = torch.where(torch.isinf(tm), torch.zeros_like(tm), tm)
        return r
    MG.run_contract(monkeypatch, work)


# ------------------------------------------------------------------------------------------------------------- the other entry points
def _extractor(dt, B, seed=4):
    from m3l_amd import MAEExtractor
    D, fs = 128, 2
    kw = dict(image_size=32, tactile_size=16, image_patch_size=8, tactile_patch_size=4, dim=D, depth=2, heads=2, mlp_dim=256,
              image_channels=3 * fs, tactile_channels=3 * fs, frame_stack=fs)
    torch.manual_seed(seed)
    mae = VTMAE(encoder=VTT(**kw), compute_dtype=dt, decoder_dim=D, decoder_depth=1, decoder_heads=2, frame_stack=fs).to(DEV)
    ext = MAEExtractor(mae, D, False, fs).to(DEV)
    g = torch.Generator().manual_seed(5)
    obs = {"image": torch.rand(B, fs, 32, 32, 3, generator=g).to(DEV), "tactile": (torch.rand(B, fs, 6, 16, 16, generator=g) * 2 - 1).to(DEV)}
    return ext, obs


@pytest.mark.parametrize("fused", [False, True], ids=["chain", "fused"])
@pytest.mark.parametrize("dt", ["fp32", "bf16"])
def test_mae_extractor(monkeypatch, dt, fused):
    """MAEExtractor (vt_load inside): forward only at B = 8 (the rollout path), forward + backward at B = 37."""
    monkeypatch.setattr(Fn, "FUSED_EXTRACTOR", fused)
    ext, obs = _extractor(dt, 8)

    def rollout(g):
        with torch.no_grad():
            f = ext(obs)
        g.check("after the forward")
        return {"features": f}
    MG.run_contract(monkeypatch, rollout)
    ext, obs = _extractor(dt, 37)

    def train(g):
        ext.zero_grad(set_to_none=True)
        f = ext(obs)
        g.check("after the forward")
        f.square().mean().backward()
        g.check("after the backward")
        return {"features": f, "grad": _grads(ext)}
    MG.run_contract(monkeypatch, train)


@pytest.mark.parametrize("dt", ["fp32", "bf16"])
def test_dino_vtt_with_masks_and_a_register_token(monkeypatch, dt):
    torch.manual_seed(8)
    enc = m3l_amd.DinoVTT(image_size=32, tactile_size=32, image_patch_size=8, tactile_patch_size=8, dim=64, depth=2, heads=2, mlp_dim=128,
                          num_tactiles=2, num_register_tokens=1, compute_dtype=dt).to(DEV)
    g0 = torch.Generator().manual_seed(9)
    B = 5
    x = {k: torch.rand(B, 3, 32, 32, generator=g0).to(DEV) for k in ("image", "tactile1", "tactile2")}
    masks = [torch.stack([torch.randperm(16, generator=g0)[:k].sort().values for _ in range(B)]).to(DEV) for k in (9, 9)]

    def work(g):
        enc.zero_grad(set_to_none=True)
        full = enc.forward_features(x)
        out = enc(x, masks)
        g.check("after the forward")
        (out.square().mean() + full["x_norm_patchtokens"].square().mean()).backward()
        g.check("after the backward")
        return {"masked": out, "full": full["x_norm_patchtokens"], "reg": full["x_norm_regtokens"], "grad": _grads(enc)}
    MG.run_contract(monkeypatch, work)


@pytest.mark.parametrize("dt", ["fp32", "bf16"])
def test_dinov2_frozen_at_the_golden_size(monkeypatch, golden_dir, dt):
    from m3l_amd import DinoV2Frozen
    z = np.load(os.path.join(golden_dir, "dinov2_small.npz"))
    dim, depth, heads, patch, img, reg = [int(v) for v in z["meta"]]
    m = DinoV2Frozen(embed_dim=dim, depth=depth, num_heads=heads, patch_size=patch, img_size=img, num_register_tokens=reg, compute_dtype=dt)
    m.load_state_dict({k[len("param/"):]: torch.tensor(z[k]) for k in z.files if k.startswith("param/")}, strict=True)
    m = m.to(DEV)
    x = torch.tensor(z["input/x"]).to(DEV)

    def work(g):
        f = m.forward_features(x)
        g.check("after the forward")
        return {k: v for k, v in f.items() if isinstance(v, torch.Tensor)}
    MG.run_contract(monkeypatch, work)


@pytest.mark.parametrize("dt", ["fp32", "bf16"])
@pytest.mark.parametrize("P,Q,B,K", [(5, 2, 5, 4096), (10, 2, 33, 65536), (3, 2, 70, 8192)])
def test_dino_head_and_loss(monkeypatch, P, Q, B, K, dt):
    """DINOHead + DINOLoss forward / backward; B = 33 takes the second pass of the teacher-sum loop, B = 70 the second pass of the one-wave
    final kernel.  Two loss calls, so that the pending centre update (one-step delay) is applied once."""
    torch.manual_seed(K + B)
    head = m3l_amd.DINOHead(64, K, hidden_dim=128, bottleneck_dim=32, compute_dtype=dt).to(DEV)
    g0 = torch.Generator().manual_seed(B)
    x = torch.randn(P, B, 64, generator=g0).to(DEV)
    teacher = (1.5 * torch.randn(Q, B, K, generator=g0)).to(DEV)

    def work(g):
        head.zero_grad(set_to_none=True)
        crit = m3l_amd.DINOLoss(K).to(DEV)
        xg = x.clone().requires_grad_(True)
        s = head(xg)
        l0 = crit(s, teacher, 0.04)
        g.check("after the forward")
        l0.backward()
        g.check("after the backward")
        with torch.no_grad():
            l1 = crit(head(x), teacher, 0.05)
        g.check("after the second loss")
        return {"logits": s, "loss": l0, "loss_next": l1, "center": crit.center, "dx": xg.grad, "grad": _grads(head)}
    MG.run_contract(monkeypatch, work)


@pytest.mark.parametrize("dt", ["fp32", "bf16"])
def test_vtdino_step_small_configuration(monkeypatch, dt):
    g0 = torch.Generator().manual_seed(100)
    x = {k: torch.rand(4, 3, 32, 32, generator=g0).to(DEV) for k in ("image", "tactile1", "tactile2")}

    def work(g):
        torch.manual_seed(0)
        enc = m3l_amd.DinoVTT(image_size=32, tactile_size=32, image_patch_size=8, tactile_patch_size=8, dim=64, depth=2, heads=2, mlp_dim=128,
                              num_tactiles=2, num_register_tokens=1, compute_dtype=dt)
        model = m3l_amd.VTDINO(encoder=enc, dino_head=partial(m3l_amd.DINOHead, out_dim=512, hidden_dim=64, bottleneck_dim=32), optim_cfg=None,
                               lr_scheduler_cfg=None, wd_scheduler_cfg=None, local_mask_scale=(0.45, 0.6), global_mask_scale=(0.7, 1.0),
                               num_global_masks=2, num_local_masks=3, allow_mask_overlap=True, teacher_temp=0.05).to(DEV)
        model.current_teacher_temp = 0.05
        out = model.training_step(x, 0)
        g.check("after the forward")
        out["loss"].backward()
        g.check("after the backward")
        grads = _grads(model.student_encoder)
        model.on_train_batch_end(out, x, 0)
        g.check("after the teacher update")
        return {"loss": out["loss"], "grad": grads, "teacher": dict(model.teacher_encoder.named_parameters())}
    MG.run_contract(monkeypatch, work)


def test_vt_load_float_and_uint8(monkeypatch, golden_dir):
    from m3l_amd import vt_load
    zf, zu = np.load(os.path.join(golden_dir, "vt_load_fs2.npz")), np.load(os.path.join(golden_dir, "vt_load_u8.npz"))
    assert zu["in/image"].dtype == np.uint8

    def work(g):
        a = vt_load({"image": zf["in/image"], "tactile": zf["in/tactile"]}, frame_stack=2)
        b = vt_load({"image": zu["in/image"], "tactile": zu["in/tactile"]}, image_normalization=[0, 255], tactile_normalization=[-2, 3], frame_stack=2)
        g.check("after vt_load")
        return {"float": a, "u8": b}
    MG.run_contract(monkeypatch, work, need_ws=False)


@pytest.mark.parametrize("M", [1031, 13000])
def test_layernorm_fn(monkeypatch, M):
    """M = 13000: m3l_ln_bwd_blocks takes its 4-rows-per-wave branch."""
    D = 192
    g0 = torch.Generator().manual_seed(M)
    x = (torch.randn(M, D, generator=g0) * 2 + 0.5).to(DEV)
    gamma = torch.randn(D, generator=g0).to(DEV).requires_grad_(True)
    beta = torch.randn(D, generator=g0).to(DEV).requires_grad_(True)
    dy = torch.randn(M, D, generator=g0).to(DEV)

    def work(g):
        xg = x.clone().requires_grad_(True)
        y = Fn.LayerNormFn.apply(xg, gamma, beta, 1e-5)
        g.check("after the forward")
        dx, dg, db = torch.autograd.grad((y * dy).sum(), (xg, gamma, beta))
        g.check("after the backward")
        return {"y": y, "dx": dx, "dg": dg, "db": db}
    MG.run_contract(monkeypatch, work)


def test_gather_linear_act_and_concat_fns(monkeypatch):
    g0 = torch.Generator().manual_seed(3)
    B, N, D, K = 7, 48, 192, 13
    tok = torch.randn(B, N, D, generator=g0).to(DEV)
    idx = torch.stack([torch.randperm(N, generator=g0)[:K] for _ in range(B)]).to(DEV)
    M, Kin, Nout = 37, 256, 64
    x = torch.randn(M, Kin, generator=g0).to(DEV)
    w = (torch.randn(Nout, Kin, generator=g0) / 16).to(DEV).requires_grad_(True)
    b = torch.randn(Nout, generator=g0).to(DEV).requires_grad_(True)
    mask = (torch.rand(M, Nout, generator=g0) >= 0.1).to(torch.uint8).to(DEV)
    cot = torch.randn(M, Nout, generator=g0).to(DEV)
    other = torch.randn(M, 24, generator=g0).to(DEV).requires_grad_(True)

    def gather(g):
        t = tok.clone().requires_grad_(True)
        y = Fn.GatherTokensFn.apply(t, idx)
        g.check("after the gather")
        (dt,) = torch.autograd.grad(y.square().sum(), (t,))
        g.check("after the scatter")
        return {"y": y, "dx": dt}
    MG.run_contract(monkeypatch, gather, need_ws=False)

    def linear(g):
        xg = x.clone().requires_grad_(True)
        out = {}
        for name, relu, mk in (("relu_mask", True, mask), ("relu", True, None), ("plain", False, None)):
            y = Fn.LinearActFn.apply(xg, w, b, relu, mk, 1.0 / 0.9 if mk is not None else 1.0)
            cat = Fn.Concat2Fn.apply(y, other)
            g.check("after the forward")
            grads = torch.autograd.grad((cat[:, :Nout] * cot).sum() + cat[:, Nout:].sum(), (xg, w, b, other))
            g.check("after the backward")
            out[name] = {"y": y, "cat": cat, "g": list(grads)}
        return out
    MG.run_contract(monkeypatch, linear)


# ------------------------------------------------------------------------------- direct C-ABI calls with caller-chosen strides
def _gap_is_fill(g, t, width):
    """Columns width.. of every row of a caller-strided output still hold the context's fill byte (nothing to look at unguarded)."""
    if g.fill is None:
        return True
    gap = t[:, width:].contiguous().view(torch.uint8)
    return bool((gap == g.fill).all())


@pytest.mark.parametrize("code", [0, 1])
@pytest.mark.parametrize("out", ["f32", "t", "t+pre"])
@pytest.mark.parametrize("M,N,K", [(77, 48, 48), (129, 200, 776)])
def test_gemm_nt_with_ldc_wider_than_n(monkeypatch, M, N, K, out, code):
    torch.manual_seed(M + N + K)
    A = (0.3 * torch.randn(M, K, device=DEV)).to(_t(code))
    W = (0.3 * torch.randn(N, K, device=DEV)).to(_t(code))
    bias = torch.randn(N, device=DEV)
    ldc = N + 8

    def work(g):
        o32 = g.alloc((M, ldc), torch.float32, DEV) if out == "f32" else None
        ot = g.alloc((M, ldc), _t(code), DEV) if out != "f32" else None
        pre = g.alloc((M, ldc), _t(code), DEV) if out == "t+pre" else None
        L.check(L.lib().m3l_op_gemm_nt(code, L.ptr(A), K, L.ptr(W), K, M, N, K, L.ptr(bias), None, L.ptr(o32), L.ptr(ot), L.ptr(pre), None,
                                       1 if pre is not None else 0, ldc, _s()), "gemm_nt")
        g.check("after gemm_nt")
        res = {}
        for name, t in (("f32", o32), ("t", ot), ("pre", pre)):
            if t is not None:
                assert _gap_is_fill(g, t, N), f"gemm_nt wrote the columns between N and ldc of {name}"
                res[name] = t[:, :N].contiguous()
        return res
    MG.run_contract(monkeypatch, work, callers="all", need_ws=False)


@pytest.mark.parametrize("code", [0, 1])
@pytest.mark.parametrize("M,N,K", [(333, 48, 192), (300, 264, 136), (2500, 1536, 384)])
def test_gemm_tn_with_ldo_wider_than_k(monkeypatch, M, N, K, code):
    torch.manual_seed(M + N)
    Y = torch.randn(M, N, device=DEV).to(_t(code))
    X = torch.randn(M, K, device=DEV).to(_t(code))
    ldo = K + 8

    def work(g):
        nb = L.lib().m3l_op_gemm_tn_ws_bytes(M, N, K)
        ws = g.alloc((nb,), torch.uint8, DEV, kind="ws")
        o = g.alloc((N, ldo), torch.float32, DEV)
        L.check(L.lib().m3l_op_gemm_tn(code, L.ptr(Y), N, L.ptr(X), K, M, N, K, L.ptr(ws), nb, L.ptr(o), ldo, _s()), "gemm_tn")
        g.check("after gemm_tn")
        assert _gap_is_fill(g, o, K), "gemm_tn wrote the columns between K and ldo"
        return {"dW": o[:, :K].contiguous()}
    MG.run_contract(monkeypatch, work, callers="all")


def test_gemm_tn_grouped_mixed_shapes(monkeypatch):
    M, shapes = 2100, [(192, 768), (64, 32), (8, 200), (264, 136), (192, 48)]
    torch.manual_seed(M)
    cnt = len(shapes)
    Ys = [(0.5 * torch.randn(M, n, device=DEV)).to(torch.bfloat16) for n, _ in shapes]
    Xs = [(0.5 * torch.randn(M, k, device=DEV)).to(torch.bfloat16) for _, k in shapes]
    Ns, Ks = (C.c_int * cnt)(*[n for n, _ in shapes]), (C.c_int * cnt)(*[k for _, k in shapes])

    def work(g):
        nb = L.lib().m3l_op_gemm_tn_grouped_ws_bytes(1, cnt, M, Ns, Ks)
        ws = g.alloc((nb,), torch.uint8, DEV, kind="ws")
        outs = [g.alloc((n, k), torch.float32, DEV) for n, k in shapes]
        L.check(L.lib().m3l_op_gemm_tn_grouped(1, cnt, M, L.ptr_array(Ys), Ns, L.ptr_array(Xs), Ks, Ns, Ks, L.ptr_array(outs), L.ptr(ws), nb, _s()),
                "gemm_tn_grouped")
        g.check("after gemm_tn_grouped")
        return outs
    MG.run_contract(monkeypatch, work, callers="all")


@pytest.mark.parametrize("code", [0, 1])
@pytest.mark.parametrize("DH", [64, 32, 128])
@pytest.mark.parametrize("n", [10, 75, 113])
def test_attention_entry_points(monkeypatch, n, DH, code):
    B, H = 2, 3
    torch.manual_seed(n * 7 + DH)
    qkv = torch.randn(B * n, 3 * H * DH, device=DEV).to(_t(code))
    dO = torch.randn(B * n, H * DH, device=DEV).to(_t(code))
    lib = L.lib()

    def work(g):
        o = g.alloc((B * n, H * DH), _t(code), DEV)
        lse = g.alloc((B, H, n), torch.float32, DEV)
        dsum = g.alloc((B, H, n), torch.float32, DEV)
        dqkv = g.alloc((B * n, 3 * H * DH), _t(code), DEV)
        if DH == 64:
            L.check(lib.m3l_op_attn_fwd(code, L.ptr(qkv), L.ptr(o), L.ptr(lse), B, n, H, _s()), "attn_fwd")
            g.check("after attn_fwd")
            L.check(lib.m3l_op_attn_bwd(code, L.ptr(qkv), L.ptr(o), L.ptr(dO), L.ptr(lse), L.ptr(dsum), L.ptr(dqkv), B, n, H, _s()), "attn_bwd")
        else:
            L.check(lib.m3l_op_attn_fwd_dh(code, L.ptr(qkv), L.ptr(o), L.ptr(lse), B, n, H, _s(), DH), "attn_fwd_dh")
            g.check("after attn_fwd_dh")
            L.check(lib.m3l_op_attn_bwd_dh(code, L.ptr(qkv), L.ptr(o), L.ptr(dO), L.ptr(lse), L.ptr(dsum), L.ptr(dqkv), B, n, H, _s(), DH), "attn_bwd_dh")
        g.check("after the attention backward")
        return {"o": o, "lse": lse, "dsum": dsum, "dqkv": dqkv}
    MG.run_contract(monkeypatch, work, callers="all", need_ws=False)


@pytest.mark.parametrize("code", [0, 1])
@pytest.mark.parametrize("rows,cols", [(147, 128), (128, 147)])
def test_colsum_and_prep_weight(monkeypatch, rows, cols, code):
    torch.manual_seed(rows)
    src = torch.randn(rows, cols, device=DEV)
    Y = torch.randn(1000, cols, device=DEV).to(_t(code))
    lib = L.lib()

    def work(g):
        dst = g.alloc((rows, cols), _t(code), DEV)
        dstT = g.alloc((cols, rows), _t(code), DEV)
        L.check(lib.m3l_op_prep_weight(code, L.ptr(src), rows, cols, L.ptr(dst), L.ptr(dstT), _s()), "prep_weight")
        g.check("after prep_weight")
        ws = g.alloc((lib.m3l_op_colsum_ws_bytes(cols),), torch.uint8, DEV, kind="ws")
        out = g.alloc((cols,), torch.float32, DEV)
        L.check(lib.m3l_op_colsum(code, L.ptr(Y), 1000, cols, cols, L.ptr(ws), L.ptr(out), _s()), "colsum")
        g.check("after colsum")
        assert torch.equal(dst, src.to(_t(code))) and torch.equal(dstT, src.to(_t(code)).t())       # a cast and a transposed cast: exact
        return {"dst": dst, "dstT": dstT, "colsum": out}
    MG.run_contract(monkeypatch, work, callers="all")


@pytest.mark.parametrize("rows,N", [(4 * 3 * 48, 48), (2 * 113, 113), (75, 1537)])
def test_dropout_mask_kernel(monkeypatch, rows, N):
    def work(g):
        out = g.alloc((rows, N), torch.uint8, DEV)
        L.check(L.lib().m3l_op_dropout_mask(0.1, 12345678901234, 2, 3, rows, N, L.ptr(out), _s()), "dropout_mask")
        g.check("after dropout_mask")
        assert bool((out <= 1).all())
        return {"mask": out}
    MG.run_contract(monkeypatch, work, callers="all", need_ws=False)


@pytest.mark.parametrize("entry", ["adam", "adam_scaled", "adam_dev", "adamw", "adamw_clip"])
@pytest.mark.parametrize("n", [1, 1023, 4097])
def test_adam_entry_points_on_a_4_byte_aligned_view(entry, n):
    """Parameters, gradients and both moments start 4 bytes into their buffers (what a flat layout after an odd-length parameter gives
    every later one): the elements in front of and behind the view are unchanged, and — the update being element-wise — the result
    is the bits the same call gives on 16-byte aligned buffers (adamw_clip: its norm is a reduction whose grouping may follow the
    alignment, so only the neighbours and finiteness are held)."""
    lib = L.lib()
    g0 = torch.Generator().manual_seed(n)
    init = [torch.randn(n, generator=g0), torch.randn(n, generator=g0), 0.1 * torch.randn(n, generator=g0), torch.rand(n, generator=g0)]

    def run(offset):
        bufs = [torch.full((n + 8,), 7.25, device=DEV) for _ in range(4)]
        views = [b[offset:offset + n] for b in bufs]
        for v, t in zip(views, init):
            v.copy_(t)
        assert all(v.data_ptr() % 16 == 4 * offset for v in views)
        p, gr, m, v = [x.data_ptr() for x in views]
        hp = (1e-3, 0.9, 0.999, 1e-8, 0.01)
        if entry == "adam":
            L.check(lib.m3l_adam_step(p, gr, m, v, n, *hp, 3, _s()), entry)
        elif entry == "adam_scaled":
            L.check(lib.m3l_adam_step_scaled(p, gr, m, v, n, *hp, 3, 0.5, _s()), entry)
        elif entry == "adam_dev":
            step = torch.full((1,), 2, dtype=torch.int32, device=DEV)
            bc = torch.zeros(2, device=DEV)
            L.check(lib.m3l_adam_step_dev(p, gr, m, v, n, *hp, step.data_ptr(), bc.data_ptr(), _s()), entry)
            assert int(step.item()) == 3
        else:
            nws = torch.zeros(1026, device=DEV)
            L.check(lib.m3l_adamw_step(p, gr, m, v, n, *hp, 3, 0.5, 0.5 if entry == "adamw_clip" else 0.0, nws.data_ptr(), 1, _s()), entry)
        torch.cuda.synchronize()
        for b in bufs:
            assert bool((b[:offset] == 7.25).all()) and bool((b[offset + n:] == 7.25).all()), f"{entry} wrote outside its {n} elements"
        assert all(bool(torch.isfinite(x).all()) for x in views)
        return [x.clone() for x in views]

    aligned, shifted = run(0), run(1)
    assert not torch.equal(aligned[0], init[0].to(DEV))
    if entry != "adamw_clip":
        for name, a, b in zip(("params", "grads", "exp_avg", "exp_avg_sq"), aligned, shifted):
            assert torch.equal(a, b), f"{entry} n={n}: {name} differ between the aligned and the 4-byte aligned call"


# ----------------------------------------------------------------------------------------------------- direct-gradient mode
LEARNED_POS_SLOTS = {"encoder.pos_embedding", "decoder_pos_emb.weight"}
UNUSED_UNDER_LEARNED_POS = {"encoder_modality_embedding.weight", "decoder_modality_embedding.weight"}     # (the kernels add a zero table instead)


@pytest.mark.parametrize("fused", [False, True], ids=["chain", "fused"])
@pytest.mark.parametrize("sincos", [True, False], ids=["sincos", "learnedpos"])
@pytest.mark.parametrize("dt", ["bf16", "fp32"])
def test_direct_gradient_slots_are_overwritten_not_accumulated(monkeypatch, dt, sincos, fused):
    """One GradSync + FlatAdam step of the cfg-2 geometry with the flat gradient buffer holding NaN where zero_grad() would have left
    zeros.  The contract this pins (include/m3l_amd.h): m3l_mae_step_bwd (and the per-module backwards) OVERWRITE every gradient slot
    they produce — after the backward each equals the gradient autograd receives without a GradSync, bit for bit.  The only slots that
    are ADDED to are the learned position tables (use_sincosmod_encodings=False: their gradient is accumulated by autograd after the
    call), so those — and only those — must be zeroed by the caller; they are zeroed here and nothing else is.  A parameter that takes no
    gradient in the call (the modality tables under learned positions) has its slot left exactly as it was."""
    from m3l_amd.parallel import FlatAdam, GradSync
    enc_kw, mae_kw = CFG2[0], dict(CFG2[1], use_sincosmod_encodings=sincos)
    monkeypatch.setattr(Fn, "FUSED_STEP", fused)
    ref_mae, x, noises = _mae(enc_kw, mae_kw, 5, dt)
    loss_ref = ref_mae(x, mask_noise=noises)
    loss_ref.backward()
    ref = {n: p.grad.clone() for n, p in ref_mae.named_parameters() if p.grad is not None}
    before = {n: p.detach().clone() for n, p in ref_mae.named_parameters()}

    def work(g):
        mae, _, _ = _mae(enc_kw, mae_kw, 5, dt)
        sync = GradSync(mae)
        opt = FlatAdam(sync, lr=1e-3)
        sync.zero_grad()
        sync.flat.fill_(float("nan"))
        named = dict(mae.named_parameters())
        if not sincos:
            for n in LEARNED_POS_SLOTS:
                named[n].grad.zero_()
        loss = mae(x, mask_noise=noises)
        g.check("after the forward")
        loss.backward()
        sync.finish()
        g.check("after the backward")
        assert torch.equal(loss.detach(), loss_ref.detach())
        stale = sorted(n for n in ref if not bool(torch.isfinite(named[n].grad).all()))
        assert stale == [], f"gradient slots that were added to (or left unwritten) instead of overwritten: {stale}"
        untouched = []
        for n, p in named.items():
            if n in ref and not (n in LEARNED_POS_SLOTS and fused):
                assert torch.equal(p.grad, ref[n]), n
            elif n in ref:        # the library's fixed-order batch sum against torch.sum (see test_fused_step_is_bit_identical_to_module_chain)
                assert bool(p.grad.any()), n
            elif id(p) in sync._span:      # a parameter that takes no gradient in this call: its slot is left exactly as it was
                assert bool(torch.isnan(p.grad).all()), n
                untouched.append(n)
                p.grad.zero_()
            else:
                assert p.grad is None, n
        assert sorted(untouched) == ([] if sincos else sorted(UNUSED_UNDER_LEARNED_POS)), untouched
        grads = {n: p.grad.clone() for n, p in named.items() if p.grad is not None}
        opt.step()
        g.check("after the optimizer step")
        assert not torch.equal(named["to_pixels.weight"].detach(), before["to_pixels.weight"])
        return {"loss": loss, "grad": grads, "param": {n: p.detach() for n, p in named.items()}}
    MG.run_contract(monkeypatch, work)


# ------------------------------------------------------------------------------------------- the unaligned flat layout (last)
@pytest.mark.parametrize("dt", ["fp32", "bf16"])
def test_flat_buffers_with_4_byte_aligned_members(monkeypatch, dt):
    """7 x 7 RGB / 5 x 5 tactile patches: the 147-long and 75-long LayerNorm / head tensors leave every later member of GradSync's flat
    parameter and gradient buffers 4-byte aligned.  One fused direct-gradient step: loss and every gradient equal the module-path run
    (every tensor its own aligned allocation) bit for bit; the parameters after FlatAdam.step() equal torch.optim.Adam within the bound
    of test_flat_adam_matches_torch_adam."""
    from m3l_amd.parallel import FlatAdam, GradSync
    enc_kw, mae_kw = MAE_ARCHS["pd147_75"]
    ref_mae, x, noises = _mae(enc_kw, mae_kw, 3, dt)
    monkeypatch.setattr(Fn, "FUSED_STEP", False)
    loss_ref = ref_mae(x, mask_noise=noises)
    loss_ref.backward()
    ref = {n: p.grad.clone() for n, p in ref_mae.named_parameters() if p.grad is not None}
    names = [n for n, _ in ref_mae.named_parameters() if n not in GradSync.SKIP]
    assert sorted(ref) == sorted(names)
    ref_named = dict(ref_mae.named_parameters())
    torch.optim.Adam([ref_named[n] for n in names], lr=3e-3, weight_decay=0.01).step()
    monkeypatch.setattr(Fn, "FUSED_STEP", True)

    def work(g):
        mae, _, _ = _mae(enc_kw, mae_kw, 3, dt)
        sync = GradSync(mae)
        opt = FlatAdam(sync, lr=3e-3, weight_decay=0.01)
        named = dict(mae.named_parameters())
        odd = [n for n in names if named[n].data_ptr() % 16 != 0]
        assert odd and any(named[n].grad.data_ptr() % 16 != 0 for n in names), "every member of the flat buffers is 16-byte aligned: the case is stale"
        sync.zero_grad()
        loss = mae(x, mask_noise=noises)
        assert type(loss.grad_fn).__name__ == "MaeStepFnBackward"
        g.check("after the forward")
        loss.backward()
        sync.finish()
        g.check("after the backward")
        assert torch.equal(loss.detach(), loss_ref.detach())
        for n in names:
            assert torch.equal(named[n].grad, ref[n]), n
        grads = {n: named[n].grad.clone() for n in names}
        opt.step()
        g.check("after the optimizer step")
        for n in names:
            pa, pb = named[n].detach(), ref_named[n].detach()
            assert float((pa - pb).abs().max()) <= 2e-6 * max(1.0, float(pb.abs().max())), n
        return {"loss": loss, "grad": grads, "param": {n: named[n].detach() for n in names}}
    MG.run_contract(monkeypatch, work)
