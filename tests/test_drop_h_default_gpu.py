"""The default of m3l_set_drop_h on the device: the fused MAE step under unset switches (auto: the stacks of the measured families do not
save h, their fc2 weight gradient stages u and applies the GELU one ring stage ahead) gives the loss and EVERY gradient of the run that
saved h, bit for bit — at cfg-2 token counts (encoder n = 48 on the per-sample blocks, decoder n = 192), B = 3, depth 2 + 2, with the
decoder on 192-row tiles (forced at this batch) and on the 48-row tiles it takes by itself, with fp32 and bf16 residual streams."""
import ctypes as C

import pytest
import torch

from m3l_amd import VTMAE, VTT
from m3l_amd import _lib as L

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
AUTO = -1
B = 3


@pytest.fixture(scope="module")
def model_and_batch():
    torch.manual_seed(6)
    enc = VTT(image_size=64, tactile_size=32, image_patch_size=8, tactile_patch_size=4, dim=192, depth=2, heads=3, mlp_dim=768)
    mae = VTMAE(encoder=enc, decoder_dim=192, masking_ratio=0.75, decoder_depth=2, decoder_heads=3, compute_dtype="bf16").to(DEV)
    g = torch.Generator(device="cpu").manual_seed(13)
    x = {"image": torch.rand(B, 3, 64, 64, generator=g).to(DEV), "tactile1": torch.rand(B, 3, 32, 32, generator=g).to(DEV),
         "tactile2": torch.rand(B, 3, 32, 32, generator=g).to(DEV)}
    noises = [torch.rand(B, 64, generator=g).to(DEV) for _ in range(3)]
    return mae, x, noises


def step(mae, x, noises):
    mae.zero_grad(set_to_none=True)
    loss = mae(x, mask_noise=noises)
    loss.backward()
    torch.cuda.synchronize()
    return loss.detach().clone(), {n: p.grad.clone() for n, p in mae.named_parameters() if p.grad is not None}


def plans():
    lib, cfg = L.lib(), L.TfCfg(192, 2, 3, 768, 1, 1, 64)
    enc, dec = L.TfPlan(), L.TfPlan()
    L.check(lib.m3l_transformer_plan(C.byref(cfg), B, 48, None, C.byref(enc)), "plan")
    L.check(lib.m3l_transformer_plan(C.byref(cfg), B, 192, None, C.byref(dec)), "plan")
    return enc, dec


@pytest.mark.parametrize("families", [None, 3], ids=["default_families", "both_families"])
@pytest.mark.parametrize("rb", [0, 1], ids=["res_f32", "res_bf16"])
@pytest.mark.parametrize("t192", [5, 1], ids=["rows192", "rows48"])     # 5 = the tall row tiles at any row count, the encoder stays on its blocks
def test_default_matches_saved_h_bit_for_bit(model_and_batch, t192, rb, families):
    mae, x, noises = model_and_batch
    lib, res = L.lib(), []
    old = [("t192", lib.m3l_set_t192(t192)), ("residual_bf16", lib.m3l_set_residual_bf16(rb))]
    if families is not None:
        old.append(("drop_h_auto", lib.m3l_set_drop_h_auto(families)))
    try:
        for drop in (0, AUTO):
            old_d = lib.m3l_set_drop_h(drop)
            try:
                enc, dec = plans()
                assert enc.fwd_mlp == L.TF_BLOCK and dec.fwd_mlp == (L.TF_IN_TAIL if t192 == 5 else L.TF_T192)
                if drop == AUTO:
                    assert dec.h_from_u == 1, "auto covers the row tiles in every setting of this test"
                    assert families is None or enc.h_from_u == 1
                else:
                    assert enc.h_from_u == 0 and dec.h_from_u == 0
                res.append(step(mae, x, noises))
            finally:
                lib.m3l_set_drop_h(old_d)
    finally:
        for name, v in reversed(old):
            getattr(lib, "m3l_set_" + name)(v)
    (l0, g0), (l1, g1) = res
    assert torch.isfinite(l0) and torch.equal(l0, l1)
    assert g0.keys() == g1.keys() and len(g0) > 40
    for n in g0:
        assert torch.equal(g0[n], g1[n]), n
