"""Launch structure of the compute-type weight copies (prep_weights_kernel, csrc/elementwise.hip), read through the in-library profiler:
a fused chain (m3l_mae_step_fwd / m3l_extractor_fwd) issues the copies of all its modules in one launch per 64 matrices, the module chain
issues the same matrices module by module, no backward issues any, M3L_PREP_BATCH=0 gives every module of the fused chain its own launch,
and a fused step leaves no state behind that a second one could see.  Counts and torch.equal only: no tolerance anywhere."""
import ctypes as C
import json
import os
import re
import subprocess
import sys

import pytest
import torch
import torch.nn as nn

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

from m3l_amd import VTMAE, VTT, Transformer  # noqa: E402
from m3l_amd import _lib as L  # noqa: E402
from m3l_amd import functional as Fn  # noqa: E402
from m3l_amd.fusion import pooled_embeddings  # noqa: E402

DEV = "cuda:0"
B = 6
ARCHS = ["tiny_bf16", "decdim_bf16", "vision_only_fp32", "earlyconv_bf16"]


class _PrepProf:
    """launches of prep_weights inside the scope: a list of (matrices, dtype code), one entry per launch (class prep_weights[MxDx0])"""

    def __enter__(self):
        L.lib().m3l_prof_begin(b"prep_weights", 1)
        return self

    def __exit__(self, *a):
        lib = L.lib()
        lib.m3l_prof_end()
        self.launches = []
        for i in range(lib.m3l_prof_count()):
            name = C.create_string_buffer(96)
            ms, n, w, by = C.c_double(), C.c_long(), C.c_double(), C.c_double()
            lib.m3l_prof_get(i, name, 96, C.byref(ms), C.byref(n), C.byref(w), C.byref(by))
            m = re.fullmatch(r"prep_weights\[(\d+)x(\d+)x0\]", name.value.decode())
            assert m, name.value
            self.launches += [(int(m.group(1)), int(m.group(2)))] * n.value

    def matrices(self):
        return sorted(m for m, _ in self.launches)


def _build(arch, depth=3):
    """the architectures of tests/test_parity_gpu.py::test_fused_step_is_bit_identical_to_module_chain -> (mae, inputs, mask noise)"""
    kw = dict(image_size=32, tactile_size=16, image_patch_size=8, tactile_patch_size=4, dim=128, depth=depth, heads=2, mlp_dim=256)
    mkw = dict(decoder_dim=128, masking_ratio=0.75, decoder_depth=2, decoder_heads=2)
    if arch == "decdim_bf16":
        mkw.update(decoder_dim=64, decoder_heads=1)
    if arch == "vision_only_fp32":
        kw.update(num_tactiles=0)
        mkw.update(num_tactiles=0)
    if "earlyconv" in arch:
        mkw.update(early_conv_masking=True)
    dt = "fp32" if arch.endswith("fp32") else "bf16"
    torch.manual_seed(2)
    mae = VTMAE(encoder=VTT(**kw), compute_dtype=dt, **mkw)
    g = torch.Generator(device="cpu").manual_seed(11)
    x = {"image": torch.rand(B, 3, 32, 32, generator=g)}
    nt = kw.get("num_tactiles", 2)
    for i in range(nt):
        x[f"tactile{i + 1}"] = torch.rand(B, 3, 16, 16, generator=g)
    noises = [torch.rand(B, 16, generator=g) for _ in range(1 + nt)]
    return mae, x, noises


def _stack(tf):
    return tf.depth * (3 + int(tf.project_out))


def _modules(mae, head=None):
    """matrices per weight-owning module of one forward, in chain order: front end (patch embed: one per modality group present; EarlyCNN:
    four per stem present), encoder stack, enc_to_dec, then decoder stack and heads (one per group) or the extractor's head stack"""
    groups = 1 + int(mae.num_tactiles > 0)
    out = [4] * groups if mae.early_conv_masking else [groups]
    out.append(_stack(mae.encoder.transformer))
    if head is not None:
        return out + [_stack(head)]
    if isinstance(mae.enc_to_dec, nn.Linear):
        out.append(1)
    return out + [_stack(mae.decoder), groups]


def _code(mae):
    return Fn.dtype_code(mae.compute_dtype)


def _forward(mae, x, noises, fused):
    keep = Fn.FUSED_STEP
    Fn.FUSED_STEP = fused
    try:
        loss = mae({k: v.to(DEV) for k, v in x.items()}, mask_noise=[n.to(DEV) for n in noises])
        assert (type(loss.grad_fn).__name__ == "MaeStepFnBackward") == fused
    finally:
        Fn.FUSED_STEP = keep
    return loss


def test_expected_totals_of_the_architectures():
    assert [sum(_modules(_build(a)[0])) for a in ARCHS] == [24, 23, 22, 30]


@pytest.mark.parametrize("arch", ARCHS)
def test_fused_step_forward_is_one_launch(arch):
    mae, x, noises = _build(arch)
    mae = mae.to(DEV)
    with _PrepProf() as prof:
        _forward(mae, x, noises, True)
    assert prof.launches == [(sum(_modules(mae)), _code(mae))], prof.launches


@pytest.mark.parametrize("arch", ARCHS)
def test_module_chain_copies_the_same_matrices(arch):
    mae, x, noises = _build(arch)
    mae = mae.to(DEV)
    with _PrepProf() as prof:
        _forward(mae, x, noises, False)
    mods = _modules(mae)
    assert sum(prof.matrices()) == sum(mods), prof.launches
    assert len(prof.launches) >= len(mods), prof.launches
    assert {d for _, d in prof.launches} == {_code(mae)}


def test_more_than_64_matrices_take_two_launches():
    mae, x, noises = _build("tiny_bf16", depth=17)
    mae = mae.to(DEV)
    assert sum(_modules(mae)) == 80
    with _PrepProf() as prof:
        _forward(mae, x, noises, True)
    assert prof.launches == [(64, 1), (16, 1)], prof.launches


def _extractor(mae):
    head = Transformer(128, 1, 2, 64, 256)
    head.compute_dtype = mae.compute_dtype
    return head.to(DEV)


def test_fused_extractor_forward_is_one_launch():
    mae, x, _ = _build("tiny_bf16")
    mae = mae.to(DEV)
    head = _extractor(mae)
    assert Fn.FUSED_EXTRACTOR
    with _PrepProf() as prof:
        feat = pooled_embeddings(mae, head, {k: v.to(DEV) for k, v in x.items()})
    assert type(feat.grad_fn).__name__ == "ExtractorFnBackward"
    assert prof.launches == [(sum(_modules(mae, head)), 1)], prof.launches
    assert sum(_modules(mae, head)) == 18


def test_backwards_copy_no_weights():
    mae, x, noises = _build("tiny_bf16")
    mae = mae.to(DEV)
    loss = _forward(mae, x, noises, True)
    with _PrepProf() as prof:
        loss.backward()
    assert prof.launches == []
    feat = pooled_embeddings(mae, _extractor(mae), {k: v.to(DEV) for k, v in x.items()})
    with _PrepProf() as prof:
        feat.square().sum().backward()
    assert prof.launches == []


_CHILD = """
import json, sys
sys.path.insert(0, {root!r})
sys.path.insert(0, {tests!r})
import test_prep_batch_gpu as T
mae, x, noises = T._build("tiny_bf16")
mae = mae.to(T.DEV)
with T._PrepProf() as prof:
    T._forward(mae, x, noises, True)
print("LAUNCHES " + json.dumps(prof.launches))
"""


def test_prep_batch_off_gives_every_module_its_own_launch():
    """M3L_PREP_BATCH is read once per process: a fresh child runs one fused forward with it set to 0"""
    env = dict(os.environ, M3L_PREP_BATCH="0")
    r = subprocess.run([sys.executable, "-c", _CHILD.format(root=ROOT, tests=os.path.join(ROOT, "tests"))], env=env, timeout=120,
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    line = [ln for ln in r.stdout.splitlines() if ln.startswith("LAUNCHES ")][-1]
    launches = [tuple(v) for v in json.loads(line[len("LAUNCHES "):])]
    mods = _modules(_build("tiny_bf16")[0])
    assert sum(mods) == 24
    assert sorted(m for m, _ in launches) == sorted(mods), launches
    assert {d for _, d in launches} == {1}


@pytest.mark.parametrize("arch", ["tiny_bf16", "earlyconv_bf16"])
def test_two_fused_steps_on_fresh_models_are_bit_identical(arch):
    res = []
    for _ in range(2):
        mae, x, noises = _build(arch)
        mae = mae.to(DEV)
        loss = _forward(mae, x, noises, True)
        loss.backward()
        torch.cuda.synchronize()
        res.append((loss.detach().clone(), {n: (None if p.grad is None else p.grad.clone()) for n, p in mae.named_parameters()}))
    assert torch.equal(res[0][0], res[1][0])
    assert set(res[0][1]) == set(res[1][1])
    for n, a in res[0][1].items():
        b = res[1][1][n]
        assert (a is None) == (b is None), n
        assert a is None or torch.equal(a, b), n
