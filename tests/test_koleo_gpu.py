"""GPU checks of the KoLeo regulariser (m3l_op_koleo_fwd / _bwd, m3l_amd.KoLeoLoss, VTDINO(koleo_weight)).

Yardsticks: the results recorded from the reference's own KoLeoLoss in float64 (tests/golden/dino_koleo.npz) and, for the shapes made here,
the float64 restatement of tests/koleo_cases.py, which test_koleo_cpu.py pins to those records to 1e-12.  Every input satisfies
koleo_cases.neighbour_gap (test_koleo_cpu.py asserts it for each of them): the best product of every row stands 1e-4 above the next, or the
candidates are equal in any arithmetic, so the neighbour indices are compared exactly, for every row.  Bounds: loss 1e-4 max(1, |ref|) and
gradient 1e-4 of its largest entry, the bars of test_sinkhorn_gpu.py for an fp32 loss and its gradient; the reference's own float32 run sits at
6e-8 and 5.5e-7 (dino_koleo.npz, loss32_err / grad32_err), so the room is for summation order only."""
from functools import lru_cache, partial

import numpy as np
import pytest
import torch

import koleo_cases as KC
import m3l_amd
import memguard as MG
from m3l_amd import _lib as L
from m3l_amd import dino as D
from test_koleo_cpu import CASES, koleo_case
from test_vtdino_cpu import _z, build_step_module, load_step_params

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
LOSS_TOL = GRAD_TOL = 1e-4


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _run(groups):
    """groups: list of (n, D) float32 CPU tensors -> (loss 0-d f32 CPU tensor, grad (groups, n, D) CPU, indices (groups, n) CPU)."""
    x = torch.cat(groups).to(DEV).requires_grad_(True)
    keep = {}
    loss = D.KoLeoFn.apply(x, len(groups), 1e-8, keep)
    loss.backward()
    torch.cuda.synchronize()
    return loss.detach().cpu(), x.grad.cpu().view(len(groups), -1, x.shape[1]), keep["indices"].cpu()


@lru_cache(maxsize=None)
def _reference(name):
    return tuple(KC.koleo_f64(x.numpy()) for x in KC.gpu_input(name))


def _compare(what, loss, grad, idx, ref_loss, ref_grad, ref_idx):
    loss_err = abs(float(loss) - ref_loss) / max(1.0, abs(ref_loss))
    gmax = float(np.abs(ref_grad).max())
    grad_err = float(np.abs(grad.double().numpy() - ref_grad).max()) / gmax if gmax > 0 else float(grad.abs().max())
    wrong = int((idx.numpy() != ref_idx).sum())
    print(f"[{what}] loss {float(loss):.7f} ref {ref_loss:.7f} err {loss_err:.2e} (bound {LOSS_TOL:.0e})  grad err {grad_err:.2e} of the largest entry "
          f"{gmax:.3e} (bound {GRAD_TOL:.0e})  neighbours that differ: {wrong} of {idx.numel()}")
    assert wrong == 0, (what, np.nonzero(idx.numpy() != ref_idx))
    assert loss_err <= LOSS_TOL, (what, loss_err)
    assert grad_err <= GRAD_TOL, (what, grad_err)


@pytest.mark.parametrize("name", CASES)
def test_recorded_cases_against_the_reference_float64_results(name):
    """Measured on an MI355X (EXPERIMENTS.md 5.9 has every case): neighbours equal in every row of every case; loss error 5.5e-10 to 1.2e-7
    (bound 1e-4), gradient error 1.8e-7 to 6.2e-7 of the largest entry (bound 1e-4), exactly zero for the single row."""
    c = koleo_case(name)
    mod = m3l_amd.KoLeoLoss()
    runs = []
    for _ in range(2):
        x = torch.from_numpy(c["x"]).to(DEV).requires_grad_(True)
        loss = mod(x)
        loss.backward()
        torch.cuda.synchronize()
        assert loss.dtype == torch.float32 and loss.dim() == 0 and mod.last.dtype == torch.int64
        runs.append((loss.detach().cpu(), x.grad.cpu(), mod.last.cpu()))
    assert all(torch.equal(a, b) for a, b in zip(runs[0], runs[1])), "two runs differ in their bits"
    loss, grad, idx = runs[0]
    _compare(name, loss, grad, idx, float(c["loss64"]), c["grad64"], c["indices"])
    y = torch.nn.functional.normalize(torch.from_numpy(c["x"]), eps=1e-8, p=2, dim=-1).to(DEV)
    assert torch.equal(mod.pairwise_NNs_inner(y).cpu(), idx) and torch.equal(mod.pairwise_NNs_inner(torch.from_numpy(c["x"]).to(DEV)).cpu(), idx)


@pytest.mark.parametrize("name", ["planted_300x192", "planted_512x384", "planted_1030x256", "planted_4096x384"])
def test_single_group_against_the_float64_restatement(name):
    r, = _reference(name)
    loss, grad, idx = _run(KC.gpu_input(name))
    _compare(name, loss, grad[0], idx[0], r["loss"], r["grad"], r["indices"])


@pytest.mark.parametrize("name", ["randn_2x35x256", "planted_2x300x256"])
def test_two_groups_do_not_see_each_other(name):
    groups, refs = KC.gpu_input(name), _reference(name)
    loss, grad, idx = _run(groups)
    singles = [_run([x]) for x in groups]
    for v, r in enumerate(refs):
        _compare(f"{name} group {v}", singles[v][0], grad[v], idx[v], r["loss"], r["grad"], r["indices"])
        assert torch.equal(grad[v], singles[v][1][0]) and torch.equal(idx[v], singles[v][2][0]), v
    assert abs(float(loss) - sum(r["loss"] for r in refs)) <= LOSS_TOL * max(1.0, abs(sum(r["loss"] for r in refs)))
    assert torch.equal(loss, singles[0][0] + singles[1][0]), "the grouped loss is not the sum of the groups' losses to the last bit"
    again = _run(groups)
    assert all(torch.equal(a, b) for a, b in zip((loss, grad, idx), again)), "two runs differ in their bits"


def _abi_fwd(x, groups, n, Dm):
    lib = L.lib()
    M = groups * n
    e = lambda shape, dt: torch.empty(shape, dtype=dt, device=DEV)      # noqa: E731
    out = dict(y=e((M, Dm), torch.float32), norm=e((M,), torch.float32), nn=e((M,), torch.int32), nn64=e((M,), torch.int64), dist=e((M,), torch.float32),
               loss=e((1,), torch.float32))
    ws = e((int(lib.m3l_op_koleo_ws_bytes(groups, n, Dm)),), torch.uint8)
    rc = lib.m3l_op_koleo_fwd(L.ptr(x), groups, n, Dm, 1e-8, L.ptr(ws), L.ptr(out["y"]), L.ptr(out["norm"]), L.ptr(out["nn"]), L.ptr(out["nn64"]),
                              L.ptr(out["dist"]), L.ptr(out["loss"]), _stream())
    return rc, out


def test_c_abi_dloss_scales_the_gradient_exactly():
    groups = KC.gpu_input("randn_2x35x256")
    x = torch.cat(groups).to(DEV)
    rc, o = _abi_fwd(x, 2, 35, 256)
    assert rc == 0, L.last_error()
    dxs = []
    for dl in (1.0, 0.5):
        dx = torch.empty_like(x)
        dloss = torch.tensor([dl], dtype=torch.float32, device=DEV)
        rc = L.lib().m3l_op_koleo_bwd(L.ptr(dloss), L.ptr(x), L.ptr(o["y"]), L.ptr(o["norm"]), L.ptr(o["nn"]), L.ptr(o["dist"]), 2, 35, 256, 1e-8,
                                      L.ptr(dx), _stream())
        assert rc == 0, L.last_error()
        dxs.append(dx)
    torch.cuda.synchronize()
    assert float(dxs[0].abs().max()) > 0 and torch.equal(dxs[1], 0.5 * dxs[0])
    assert torch.equal(o["nn"].long(), o["nn64"])
    refs = _reference("randn_2x35x256")
    assert np.array_equal(o["nn"].cpu().numpy().reshape(2, 35), np.stack([r["indices"] for r in refs]))


@pytest.mark.parametrize("shape", [(1, 4097, 64), (1, 64, 1025), (17, 4096, 8), (65536, 1, 8), (1, 0, 8), (1, 8, 0), (0, 8, 8)])
def test_c_abi_refuses_unsupported_shapes_and_writes_nothing(shape):
    """Buffers of the shape (1, 8, 8) filled with a known value, the calls with the refused shape: an error, and every byte as it was."""
    groups, n, Dm = shape
    lib = L.lib()
    x = torch.zeros(64, dtype=torch.float32, device=DEV)
    o = dict(y=torch.full((64,), 7.0, device=DEV), norm=torch.full((8,), 7.0, device=DEV), nn=torch.full((8,), 7, dtype=torch.int32, device=DEV),
             nn64=torch.full((8,), 7, dtype=torch.int64, device=DEV), dist=torch.full((8,), 7.0, device=DEV), loss=torch.full((1,), 7.0, device=DEV),
             dx=torch.full((64,), 7.0, device=DEV))
    ws = torch.full((int(lib.m3l_op_koleo_ws_bytes(1, 8, 8)),), 0x5A, dtype=torch.uint8, device=DEV)
    assert lib.m3l_op_koleo_ws_bytes(groups, n, Dm) <= ws.numel()
    rc = lib.m3l_op_koleo_fwd(L.ptr(x), groups, n, Dm, 1e-8, L.ptr(ws), L.ptr(o["y"]), L.ptr(o["norm"]), L.ptr(o["nn"]), L.ptr(o["nn64"]),
                              L.ptr(o["dist"]), L.ptr(o["loss"]), _stream())
    assert rc != 0 and "koleo_fwd" in L.last_error() and "unsupported shape" in L.last_error()
    rc = lib.m3l_op_koleo_bwd(L.ptr(o["loss"]), L.ptr(x), L.ptr(o["y"]), L.ptr(o["norm"]), L.ptr(o["nn"]), L.ptr(o["dist"]), groups, n, Dm, 1e-8,
                              L.ptr(o["dx"]), _stream())
    assert rc != 0 and "koleo_bwd" in L.last_error() and "unsupported shape" in L.last_error()
    torch.cuda.synchronize()
    assert all(bool((t == 7).all()) for t in o.values()) and bool((ws == 0x5A).all())


def _max_rel(got, ref):
    return float(np.abs(got - ref).max()) / max(1e-30, float(np.abs(ref).max()))


def _rel_l2(got, ref):
    return float(np.linalg.norm((got - ref).ravel())) / max(1e-30, float(np.linalg.norm(ref.ravel())))


@pytest.mark.parametrize("dt", ["fp32", "bf16"])
def test_two_steps_with_koleo_against_reference_fixture(dt):
    """Two consecutive steps of VTDINO(koleo_weight=0.1) from the fixture's parameters: per-view neighbours, total / DINO / KoLeo losses, logits
    and every student gradient.  Bounds as test_vtdino_gpu.py::test_two_steps_against_reference_fixture: fp32 loss 1e-4 relative, gradients 2e-3
    of the largest entry; bf16 twice the recorded error of the bf16-operand emulation.  The fixture's generator chose the inputs so that the
    float64 margin of every neighbour is at least 10 times the product error of the emulation (margin/...), so the indices are compared
    exactly in both modes.  Measured on an MI355X (step 1 / step 2; bound in brackets):
      fp32  loss rel 2.0e-7 / 3.3e-7 (1e-4)  KoLeo term 1.5e-8 / 9.8e-9 (1e-4)  grad max-rel 1.1e-6 / 2.6e-6 (2e-3)
      bf16  loss rel 5.2e-4 / 2.5e-3 (1.1e-3 / 4.3e-3)  grad max-rel 1.1e-2 / 2.4e-2 (2.1e-2 / 3.4e-2)  rel-L2 8.9e-3 / 1.6e-2 (1.8e-2 / 2.9e-2)
            logits 2.4e-3 / 4.4e-3 (4.8e-3 / 9.0e-3)"""
    z = _z("vtdino_koleo_step.npz")
    zi = _z("vtdino_koleo_step_inputs.npz")
    w = float(z["meta/koleo_weight"])
    model = build_step_module(z, compute_dtype=dt, koleo_weight=w)
    load_step_params(model, z)
    model = model.to(DEV)
    x = {k: torch.from_numpy(zi["input/" + k]).to(DEV) for k in ("image", "tactile1", "tactile2")}
    lr = float(z["meta/lr"])
    for s in range(1, int(z["meta/steps"]) + 1):
        zs = _z(f"vtdino_koleo_step_s{s}.npz")
        for p in model.parameters():
            p.grad = None
        out = model.training_step(x, s - 1)
        out["loss"].backward()
        torch.cuda.synchronize()
        assert set(out) == {"ssl_loss", "dino_loss", "koleo_loss", "loss", "online_probes_loss"}
        assert all(isinstance(out[k], float) for k in ("ssl_loss", "dino_loss", "koleo_loss")) and float(out["loss"]) == out["ssl_loss"]
        assert abs(out["dino_loss"] + out["koleo_loss"] - out["ssl_loss"]) <= 1e-6 * abs(out["ssl_loss"])
        ref_loss, ref_dino, ref_koleo = (float(z[f"step{s}/{k}"]) for k in ("loss", "dino_loss", "koleo_loss"))
        loss_rel = abs(out["ssl_loss"] - ref_loss) / abs(ref_loss)
        koleo_err = abs(out["koleo_loss"] - ref_koleo) / max(1.0, abs(ref_koleo))
        idx = model.last["koleo_indices"].cpu().numpy()
        named = dict(model.student_encoder.named_parameters())
        grad_names = [k[len("grad/"):] for k in zs.files if k.startswith("grad/")]
        emax = {n: _max_rel(named[n].grad.cpu().numpy(), zs["grad/" + n]) for n in grad_names}
        el2 = {n: _rel_l2(named[n].grad.cpu().numpy(), zs["grad/" + n]) for n in grad_names}
        s_err = float(np.abs(model.last["student_logits"].cpu().numpy() - zs["student_logits"]).max())
        t_err = float(np.abs(model.last["teacher_logits"].cpu().numpy() - zs["teacher_logits"]).max())
        if dt == "fp32":
            b_loss, b_max, b_l2 = 1e-4, 2e-3, None
            b_s = b_t = 1e-4 + 1e-3 * float(np.abs(zs["student_logits"]).max())
        else:
            pre = f"bf16emu/step{s}/"
            b_loss, b_max, b_l2 = 2 * float(z[pre + "loss_rel"]), 2 * float(z[pre + "grad_max_rel"].max()), 2 * float(z[pre + "grad_rel_l2"].max())
            b_s, b_t = 2 * float(z[pre + "student_logits_max_abs"]), 2 * float(z[pre + "teacher_logits_max_abs"])
        worst = max(emax, key=emax.get)
        print(f"[{dt}] step {s}: loss {out['ssl_loss']:.6f} ref {ref_loss:.6f} rel {loss_rel:.3e} (bound {b_loss:.3e})  dino {out['dino_loss']:.6f} ref "
              f"{ref_dino:.6f}  koleo {out['koleo_loss']:.6f} ref {ref_koleo:.6f} err {koleo_err:.2e}  grad max-rel worst {emax[worst]:.3e} at {worst} "
              f"(bound {b_max:.3e})  rel-L2 worst {max(el2.values()):.3e} (bound {b_l2})  logits max-abs student {s_err:.3e} (bound {b_s:.3e}) "
              f"teacher {t_err:.3e} (bound {b_t:.3e})  neighbours that differ: {int((idx != z[f'step{s}/koleo_indices']).sum())}")
        assert idx.shape == (2, 6) and np.array_equal(idx, z[f"step{s}/koleo_indices"]), (s, idx, z[f"step{s}/koleo_indices"])
        assert loss_rel <= b_loss, (s, loss_rel, b_loss)
        if dt == "fp32":
            assert koleo_err <= LOSS_TOL, (s, koleo_err)
        assert s_err <= b_s and t_err <= b_t, (s, s_err, b_s, t_err, b_t)
        for n in grad_names:
            assert emax[n] <= b_max, (s, n, emax[n], b_max)
            if b_l2 is not None:
                assert el2[n] <= b_l2, (s, n, el2[n], b_l2)
        for u in z[f"step{s}/unused_params"]:
            assert named[str(u)].grad is None, u
        assert all(p.grad is None for p in model.teacher_encoder.parameters()), "the teacher received a gradient"
        with torch.no_grad():
            for p in model.student_encoder.parameters():
                if p.grad is not None:
                    p.sub_(lr * p.grad)
        model.on_train_batch_end(out, x, s - 1)


def test_weight_zero_is_the_step_without_koleo():
    z = _z("vtdino_step.npz")
    x = {k: torch.from_numpy(z["input/" + k]).to(DEV) for k in ("image", "tactile1", "tactile2")}
    outs = []
    for kw in ({}, {"koleo_weight": 0.0}):
        model = build_step_module(z, **kw)
        load_step_params(model, z)
        model = model.to(DEV)
        out = model.training_step(x, 0)
        out["loss"].backward()
        torch.cuda.synchronize()
        assert set(out) == {"ssl_loss", "loss", "online_probes_loss"} and "koleo_indices" not in model.last
        outs.append((out["ssl_loss"], {n: p.grad.clone() for n, p in model.student_encoder.named_parameters() if p.grad is not None}))
    ref = float(z["step1/loss"])
    assert abs(outs[1][0] - ref) <= 1e-4 * abs(ref)
    assert outs[0][0] == outs[1][0] and outs[0][1].keys() == outs[1][1].keys()
    assert all(torch.equal(outs[0][1][n], outs[1][1][n]) for n in outs[0][1])


@pytest.mark.parametrize("name", ["contract_2x35x192", "contract_1x130x50"])
def test_memory_contract_of_the_op(monkeypatch, name):
    groups = KC.gpu_input(name)
    x0 = torch.cat(groups).to(DEV)

    def work(g):
        x = x0.clone().requires_grad_(True)
        keep = {}
        loss = D.KoLeoFn.apply(x, len(groups), 1e-8, keep)
        g.check("after the forward")
        loss.backward()
        g.check("after the backward")
        return {"loss": loss, "grad": x.grad, "indices": keep["indices"]}
    counts = MG.run_contract(monkeypatch, work)
    assert counts[0] == counts[1] and counts[0][0] == 1


def test_memory_contract_of_a_step_with_koleo(monkeypatch):
    g0 = torch.Generator().manual_seed(100)
    x = {k: torch.rand(4, 3, 32, 32, generator=g0).to(DEV) for k in ("image", "tactile1", "tactile2")}

    def work(g):
        torch.manual_seed(0)
        enc = m3l_amd.DinoVTT(image_size=32, tactile_size=32, image_patch_size=8, tactile_patch_size=8, dim=64, depth=2, heads=2, mlp_dim=128,
                              num_tactiles=2, num_register_tokens=1)
        model = m3l_amd.VTDINO(encoder=enc, dino_head=partial(m3l_amd.DINOHead, out_dim=512, hidden_dim=64, bottleneck_dim=32), optim_cfg=None,
                               lr_scheduler_cfg=None, wd_scheduler_cfg=None, local_mask_scale=(0.45, 0.6), global_mask_scale=(0.7, 1.0),
                               num_global_masks=2, num_local_masks=3, allow_mask_overlap=True, teacher_temp=0.05, koleo_weight=0.1).to(DEV)
        model.current_teacher_temp = 0.05
        out = model.training_step(x, 0)
        g.check("after the forward")
        out["loss"].backward()
        g.check("after the backward")
        grads = {n: p.grad for n, p in model.student_encoder.named_parameters() if p.grad is not None}
        return {"loss": out["loss"], "koleo": out["koleo_loss"], "indices": model.last["koleo_indices"], "grad": grads}
    MG.run_contract(monkeypatch, work)
