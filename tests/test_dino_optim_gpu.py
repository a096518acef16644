"""GPU checks of the DINO optimizer stack: m3l_dino_opt_step through the C ABI against torch.optim.AdamW + clip_grad_norm_ on separate
tensors, its exact contracts (idle segments, the teacher's moving average, m3l_adamw_step's bits, repeatability, the memory contract), and
DinoAdamW on the VTDINO step module against the reference trainer's loop body driven by torch's optimizer.

Bounds (the project's own, tests/test_parity_gpu.py test_fused_adamw_clip_matches_torch): parameters 2e-5 max|p| + 2e-6, norm 1e-5 relative,
the gradient left behind 1e-4 max|g|.  Moments: 1e-5 of their largest entry — each is two or three f32 operations per step on identical
inputs, the difference comes from contraction and the last bits of the clip coefficient, about 1e-7."""
import copy
import ctypes as C
from functools import partial

import pytest
import torch

import m3l_amd
from m3l_amd import _lib as L
from m3l_amd.parallel import GradSync
from test_vtdino_cpu import _z, build_step_module, load_step_params

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
B1, B2, EPS = 0.9, 0.999, 1e-8
SHAPES = {
    # lengths of the segments (groups alternate 0 / 1), idle segments
    "a": ([1, 3, 4, 5, 4095, 4096, 4097, 2, 8193, 7], (0, 4, 9)),        # n = 24503: boundaries off the quads, segments over several blocks
    "b": ([1 + i % 7 for i in range(40)], (0, 5, 6, 39)),                # 40 segments inside one block; two idle neighbours of different groups
    "c": ([5], ()),                                                      # S = 1, n = 5
}
HYPER = [((1e-3, 5e-4), (0.05, 0.0)), ((8e-4, 2e-3), (0.1, 0.0)), ((3e-4, 1e-3), (0.4, 0.01))]      # per step: (lr of both groups), (wd of both)
CLIPS = {"bites": 0.5, "idle": 1e6, "absent": None}


def _s():
    return torch.cuda.current_stream().cuda_stream


def _layout(shape):
    lengths, idle = SHAPES[shape]
    starts = [0]
    for ln in lengths:
        starts.append(starts[-1] + ln)
    groups = [-1 if i in idle else i % 2 for i in range(len(lengths))]
    return lengths, starts, groups


_DATA = {}


def _data(shape):
    """Initial parameters, a teacher, and three steps of gradients (zeros in the idle segments), on the CPU; made once per shape."""
    if shape not in _DATA:
        lengths, starts, groups = _layout(shape)
        g = torch.Generator().manual_seed(len(lengths))
        n = starts[-1]
        p0, t0 = torch.randn(n, generator=g), torch.randn(n, generator=g)
        grads = []
        for _ in HYPER:
            gr = torch.randn(n, generator=g)
            for i, k in enumerate(groups):
                if k < 0:
                    gr[starts[i]:starts[i + 1]] = 0.0
            grads.append(gr)
        _DATA[shape] = (p0, t0, grads)
    return _DATA[shape]


def opt_step(p, g, m, v, t, n, seg_start, seg_group, lr, wd, step, max_norm, nws, beta=0.0, gscale=1.0):
    G = len(lr)
    return L.lib().m3l_dino_opt_step(p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), None if t is None else t.data_ptr(), n,
                                     seg_start.data_ptr(), seg_group.data_ptr(), seg_group.numel(), (C.c_float * G)(*lr), (C.c_float * G)(*wd), G,
                                     B1, B2, EPS, step, gscale, 0.0 if max_norm is None else max_norm, None if nws is None else nws.data_ptr(),
                                     1, beta, _s())


def run_flat(shape, max_norm, teacher=False, hyper=HYPER, groups=None, beta=0.97):
    """Three steps of the flat launch.  -> per step clones of params, grads, both moments, the norm, the teacher, and the parameters the
    moving average read."""
    lengths, starts, lay_groups = _layout(shape)
    groups = lay_groups if groups is None else groups
    p0, t0, grads = _data(shape)
    n = starts[-1]
    p, m, v = p0.to(DEV), torch.zeros(n, device=DEV), torch.zeros(n, device=DEV)
    t = t0.to(DEV) if teacher else None
    ss, sg = torch.tensor(starts, dtype=torch.int64, device=DEV), torch.tensor(groups, dtype=torch.int32, device=DEV)
    nws = torch.zeros(1026, device=DEV)
    out = []
    for i, (lr, wd) in enumerate(hyper):
        g = grads[i].to(DEV)
        L.check(opt_step(p, g, m, v, t, n, ss, sg, lr, wd, i + 1, max_norm, nws, beta=beta), "m3l_dino_opt_step")
        out.append(dict(p=p.clone(), g=g.clone(), m=m.clone(), v=v.clone(), norm=float(nws[1025]), coef=float(nws[1024]),
                        t=None if t is None else t.clone()))
    torch.cuda.synchronize()
    return out


_REF = {}


def run_torch(shape, max_norm):
    """The same three steps on separate tensors per segment: torch.optim.AdamW(two groups, foreach=False) + clip_grad_norm_; the idle tensors
    have .grad = None.  Computed once per (shape, clip) and shared."""
    key = (shape, max_norm)
    if key not in _REF:
        lengths, starts, groups = _layout(shape)
        p0, _, grads = _data(shape)
        ps = [torch.nn.Parameter(p0[a:b].clone().to(DEV)) for a, b in zip(starts, starts[1:])]
        by_group = [[q for i, q in enumerate(ps) if i % 2 == k] for k in (0, 1)]
        opt = torch.optim.AdamW([{"params": by_group[0]}, {"params": by_group[1]}] if by_group[1] else [{"params": by_group[0]}],
                                lr=1e-3, betas=(B1, B2), eps=EPS, foreach=False)
        out = []
        for i, (lr, wd) in enumerate(HYPER):
            for k, grp in enumerate(opt.param_groups):
                grp["lr"], grp["weight_decay"] = lr[k], wd[k]
            for j, q in enumerate(ps):
                q.grad = None if groups[j] < 0 else grads[i][starts[j]:starts[j + 1]].clone().to(DEV)
            norm = float(torch.nn.utils.clip_grad_norm_(ps, max_norm, foreach=False)) if max_norm is not None else None
            opt.step()
            rec = dict(p=[q.detach().clone() for q in ps], g=[None if q.grad is None else q.grad.clone() for q in ps], norm=norm,
                       m=[opt.state[q]["exp_avg"].clone() if q in opt.state and opt.state[q] else None for q in ps],
                       v=[opt.state[q]["exp_avg_sq"].clone() if q in opt.state and opt.state[q] else None for q in ps])
            out.append(rec)
        _REF[key] = out
    return _REF[key]


def _within_param_bound(got, ref, what):
    scale = float(ref.abs().max()) + 1e-12
    err = float((got - ref).abs().max())
    assert err <= 2e-5 * scale + 2e-6, (what, err, scale)


# -------------------------------------------------------------------------------------------------------------- kernel against torch
@pytest.mark.parametrize("clip", list(CLIPS))
@pytest.mark.parametrize("shape", list(SHAPES))
def test_kernel_matches_torch_adamw_with_clip(shape, clip):
    max_norm = CLIPS[clip]
    lengths, starts, groups = _layout(shape)
    p0 = _data(shape)[0].to(DEV)
    got, ref = run_flat(shape, max_norm), run_torch(shape, max_norm)
    for i, (f, r) in enumerate(zip(got, ref)):
        if max_norm is not None:
            assert abs(f["norm"] - r["norm"]) <= 1e-5 * r["norm"], (i, f["norm"], r["norm"])
            assert (f["coef"] < 1.0) == (clip == "bites"), (i, f["coef"])
        for j, (a, b) in enumerate(zip(starts, starts[1:])):
            if groups[j] < 0:
                assert torch.equal(f["p"][a:b], p0[a:b]), f"step {i}: idle segment {j} was changed"
                assert torch.equal(r["p"][j], p0[a:b])
                assert float(f["m"][a:b].abs().max()) == 0.0 and float(f["v"][a:b].abs().max()) == 0.0, f"step {i}: idle segment {j} has moments"
                continue
            _within_param_bound(f["p"][a:b], r["p"][j], (shape, clip, i, j))
            for name in ("m", "v"):
                top = float(r[name][j].abs().max())
                assert float((f[name][a:b] - r[name][j]).abs().max()) <= 1e-5 * top, (name, shape, clip, i, j)
            if max_norm is not None:
                gs = float(r["g"][j].abs().max()) + 1e-12
                assert float((f["g"][a:b] - r["g"][j]).abs().max()) <= 1e-4 * gs, ("grad", shape, clip, i, j)


# ----------------------------------------------------------------------------------------------------------------------- exact checks
@pytest.mark.parametrize("shape", list(SHAPES))
def test_teacher_average_is_bit_equal_to_the_ema_launch_after_the_step(shape):
    """With a teacher the launch gives the bits of m3l_op_ema(teacher, post-step parameters), idle segments included, and the student side is
    the bits of the launch without a teacher."""
    beta = 0.97
    with_t, without = run_flat(shape, 0.5, teacher=True, beta=beta), run_flat(shape, 0.5)
    t = _data(shape)[1].to(DEV)
    n = t.numel()
    for i, (f, w) in enumerate(zip(with_t, without)):
        for k in ("p", "g", "m", "v"):
            assert torch.equal(f[k], w[k]), (i, k)
        src = f["p"].clone()
        L.check(L.lib().m3l_op_ema(L.ptr_array([t]), L.ptr_array([src]), (C.c_long * 1)(n), 1, beta, 1.0 - beta, _s()), "m3l_op_ema")
        assert torch.equal(f["t"], t), f"step {i}: the fused moving average differs from m3l_op_ema"
    assert not torch.equal(t, _data(shape)[1].to(DEV))


def test_uniform_hyper_parameters_against_adamw_step():
    """No idle segment, both groups on one lr / wd, against m3l_adamw_step on copies.  The two kernels share the per-element update and the
    reduction, so the norm, the coefficient and the clipped gradients are the same bits.  Parameters and moments are NOT: m3l_adamw_step
    takes float betas and forms 1 - beta2 in f32 (1.0f - 0.999f = 0.9999871e-3), m3l_dino_opt_step forms it in double as torch does
    ((float)(1 - 0.999) = 1.0000000e-3), and m3l_adamw_step's bits were to stay.  The 1.3e-5 between the two factors is carried by the
    second moment, so that is held to the parameter bound's relative part (2e-5 of its largest entry); parameters to the parameter bound,
    the first moment to the moments' 1e-5."""
    shape = "a"
    lengths, starts, _ = _layout(shape)
    hyper = [((1e-3, 1e-3), (0.05, 0.05)), ((7e-4, 7e-4), (0.2, 0.2)), ((2e-4, 2e-4), (0.0, 0.0))]
    got = run_flat(shape, 0.5, hyper=hyper, groups=[i % 2 for i in range(len(lengths))])
    p0, _, grads = _data(shape)
    n = starts[-1]
    p, m, v, nws = p0.to(DEV), torch.zeros(n, device=DEV), torch.zeros(n, device=DEV), torch.zeros(1026, device=DEV)
    for i, (lr, wd) in enumerate(hyper):
        g = grads[i].to(DEV)
        L.check(L.lib().m3l_adamw_step(p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), n, lr[0], B1, B2, EPS, wd[0], i + 1, 1.0, 0.5,
                                       nws.data_ptr(), 1, _s()), "m3l_adamw_step")
        assert torch.equal(got[i]["g"], g), (i, "clipped gradients")
        assert got[i]["norm"] == float(nws[1025]) and got[i]["coef"] == float(nws[1024]) < 1.0
        _within_param_bound(got[i]["p"], p, (i, "p"))
        assert float((got[i]["m"] - m).abs().max()) <= 1e-5 * float(m.abs().max()), (i, "m")
        assert float((got[i]["v"] - v).abs().max()) <= 2e-5 * float(v.abs().max()), (i, "v")


def test_two_runs_give_the_same_bits():
    a, b = run_flat("a", 0.5, teacher=True), run_flat("a", 0.5, teacher=True)
    for i, (x, y) in enumerate(zip(a, b)):
        assert x["norm"] == y["norm"]
        for k in ("p", "g", "m", "v", "t"):
            assert torch.equal(x[k], y[k]), (i, k)


# ------------------------------------------------------------------------------------------------------------------- memory contract
SENTINEL = 7.25


def test_memory_contract_sentinels_stale_workspace_and_misaligned_base():
    """Shape (a), n = 24503 (not a multiple of 4): all five buffers, the workspace and both tables sit 32 bytes into sentinel-filled blocks;
    the sentinels on both sides are intact after the call, a NaN-filled norm workspace gives the bits a zeroed one gives, and a base pointer
    that is only 4-byte aligned is refused with nothing written."""
    lengths, starts, groups = _layout("a")
    p0, t0, grads = _data("a")
    n, off = starts[-1], 8
    assert n % 4 == 3

    def embed(src, fill=SENTINEL, dtype=torch.float32):
        block = torch.full((src.numel() + 2 * off,), fill, dtype=dtype, device=DEV)
        view = block[off:off + src.numel()]
        view.copy_(src)
        return block, view

    def run(ws_fill):
        blocks, views = zip(*[embed(x) for x in (p0, grads[0], torch.zeros(n), torch.zeros(n), t0, torch.full((1026,), ws_fill))])
        tb, tv = zip(*[embed(torch.tensor(starts), -7, torch.int64), embed(torch.tensor(groups), -7, torch.int32)])
        p, g, m, v, t, nws = views
        assert all(x.data_ptr() % 16 == 0 for x in (p, g, m, v, t))
        L.check(opt_step(p, g, m, v, t, n, tv[0], tv[1], (1e-3, 5e-4), (0.05, 0.0), 2, 0.5, nws, beta=0.9), "m3l_dino_opt_step")
        torch.cuda.synchronize()
        for name, b, x in zip(("params", "grads", "exp_avg", "exp_avg_sq", "teacher", "norm_ws"), blocks, views):
            assert bool((b[:off] == SENTINEL).all()) and bool((b[off + x.numel():] == SENTINEL).all()), f"wrote outside {name}"
        for b, x, src in zip(tb, tv, (starts, groups)):
            assert bool((b[:off] == -7).all()) and bool((b[off + x.numel():] == -7).all()) and x.tolist() == src, "a segment table was written"
        assert all(bool(torch.isfinite(x).all()) for x in (p, g, m, v, t))
        return [x.clone() for x in (p, g, m, v, t)] + [nws[1024:].clone()]

    zeroed, stale = run(0.0), run(float("nan"))
    assert not torch.equal(zeroed[0], p0.to(DEV)) and float(zeroed[5][0]) < 1.0
    for name, a, b in zip(("params", "grads", "exp_avg", "exp_avg_sq", "teacher", "coefficient / norm"), zeroed, stale):
        assert torch.equal(a, b), f"{name} depend on what the norm workspace held before the call"

    # a 4-byte aligned base: an error code, and every block as it was
    for which in range(5):
        srcs = [p0, grads[0], torch.zeros(n), torch.zeros(n), t0]
        blocks, views = [], []
        for i, x in enumerate(srcs):
            o = off + (1 if i == which else 0)
            block = torch.full((n + 2 * off + 4,), SENTINEL, device=DEV)
            block[o:o + n].copy_(x)
            blocks.append(block)
            views.append(block[o:o + n])
        nws = torch.zeros(1026, device=DEV)
        before = [b.clone() for b in blocks]
        ss, sg = torch.tensor(starts, dtype=torch.int64, device=DEV), torch.tensor(groups, dtype=torch.int32, device=DEV)
        assert opt_step(*views, n, ss, sg, (1e-3, 5e-4), (0.05, 0.0), 2, 0.5, nws, beta=0.9) != 0
        assert "aligned" in L.last_error()
        torch.cuda.synchronize()
        assert all(torch.equal(a, b) for a, b in zip(before, blocks)) and float(nws.abs().max()) == 0.0, "a refused call wrote something"


# --------------------------------------------------------------------------------------------------------------------------- module
SCHED = dict(lr_scheduler_cfg=partial(m3l_amd.WarmupCosineScheduler, start_lr=1e-5, warmup_epochs=1, final_lr=1e-6),
             wd_scheduler_cfg=partial(m3l_amd.CosineWDSchedule, ref_weight_decay=0.05, final_weight_decay=0.4))


def _step_module(optim_cfg, **over):
    z = _z("vtdino_step.npz")
    model = build_step_module(z, compute_dtype="fp32", optim_cfg=optim_cfg, **over)
    load_step_params(model, z)
    x = {k: torch.from_numpy(z["input/" + k]).to(DEV) for k in ("image", "tactile1", "tactile2")}
    return model.to(DEV), x


def _backward(model, x, i):
    out = model.training_step(x, i)
    out["loss"].backward()
    return out


def test_module_three_iterations_against_torch_adamw_clip_schedulers_and_unfused_average():
    """The trainer's loop body (training_step + backward, clip, step, zero_grad, on_train_batch_end, lr scheduler, wd scheduler) three times:
    DinoAdamW with the teacher bound against torch.optim.AdamW + clip_grad_norm_ + the unfused moving average on a module with the same
    parameters, both under the same two schedulers and a decay schedule (0.9 -> 1.0)."""
    probe, x = _step_module(None)
    _backward(probe, x, 0)
    norm0 = float(torch.nn.utils.clip_grad_norm_([p for p in probe.parameters() if p.grad is not None], 1e9))
    g = 0.5 * norm0                                   # below the first step's norm: the clip bites
    decay = (0.9, 1.0)
    fus, _ = _step_module(partial(m3l_amd.DinoAdamW, lr=5e-4, weight_decay=0.05, max_grad_norm=g), moving_average_decay=decay, **SCHED)
    ref, _ = _step_module(partial(torch.optim.AdamW, lr=5e-4, weight_decay=0.05), moving_average_decay=decay, **SCHED)
    init = {k: v.detach().clone() for k, v in fus.named_parameters()}
    keys = list(fus.state_dict())
    opt_f, lr_f, wd_f = fus.configure_optimizers(5, 3)
    opt_r, lr_r, wd_r = ref.configure_optimizers(5, 3)
    assert isinstance(opt_f, m3l_amd.DinoAdamW) and isinstance(lr_f["scheduler"], m3l_amd.WarmupCosineScheduler)
    opt_f.bind_teacher(fus)
    assert list(fus.state_dict()) == keys and all(torch.equal(v, init[k]) for k, v in fus.named_parameters()), "re-homing changed a value or a key"
    betas_r, draw = [], ref.next_moving_average_decay
    ref.next_moving_average_decay = lambda: (betas_r.append(draw()), betas_r[-1])[1]
    betas_f = []
    ref_params = [p for p in ref.parameters() if p.requires_grad]
    pos = "student_encoder.backbone.pos_embedding"
    for i in range(3):
        out_f = _backward(fus, x, i)
        opt_f.step()
        opt_f.zero_grad()
        teacher_after_step = [p.detach().clone() for p in fus.teacher_encoder.parameters()]
        fus.on_train_batch_end(out_f, x, i)
        assert not fus._ema_in_step and all(torch.equal(a, b) for a, b in zip(teacher_after_step, fus.teacher_encoder.parameters())), \
            "on_train_batch_end applied the average a second time"
        lr_f["scheduler"].step()
        wd_f["wd_scheduler"].step()
        betas_f.append(opt_f.last_ema_beta)

        out_r = _backward(ref, x, i)
        norm_r = float(torch.nn.utils.clip_grad_norm_(ref_params, g))
        opt_r.step()
        opt_r.zero_grad()
        ref.on_train_batch_end(out_r, x, i)
        lr_r["scheduler"].step()
        wd_r["wd_scheduler"].step()

        assert abs(out_f["ssl_loss"] - out_r["ssl_loss"]) <= 1e-4 * abs(out_r["ssl_loss"]), (i, out_f["ssl_loss"], out_r["ssl_loss"])
        if i == 0:                                        # same parameters, same inputs: the norm of the probe, and the clip bites in both
            assert norm_r > g and float(opt_f.last_grad_norm) > g
            assert abs(float(opt_f.last_grad_norm) - norm_r) <= 1e-5 * norm_r, (float(opt_f.last_grad_norm), norm_r)
        assert [gr["lr"] for gr in opt_f.param_groups] == [gr["lr"] for gr in opt_r.param_groups]
        assert [gr["weight_decay"] for gr in opt_f.param_groups] == [gr["weight_decay"] for gr in opt_r.param_groups]
        named_r = dict(ref.named_parameters())
        for k, p in fus.named_parameters():
            _within_param_bound(p.detach(), named_r[k].detach(), (i, k))
        assert torch.equal(dict(fus.named_parameters())[pos].detach(), init[pos]) and torch.equal(named_r[pos].detach(), init[pos]), \
            "pos_embedding (never used by the forward) was changed"
        assert fus.current_teacher_temp == ref.current_teacher_temp
    assert betas_f == betas_r == [0.9 + i * (1.0 - 0.9) / 15 for i in range(3)]
    assert opt_f.param_groups[0]["weight_decay"] > 0.05 and opt_f.param_groups[1]["weight_decay"] == 0.0
    # a batch without an optimizer step (gradient accumulation): the unfused average, once, with the next decay
    before = [p.detach().clone() for p in fus.teacher_encoder.parameters()]
    fus.on_train_batch_end(out_f, x, 3)
    beta = 0.9 + 3 * (1.0 - 0.9) / 15
    changed = 0
    for t0, t1, s in zip(before, fus.teacher_encoder.parameters(), fus.student_encoder.parameters()):
        assert torch.equal(t1.detach(), t0 * beta + (1 - beta) * s.detach())
        changed += int(not torch.equal(t1.detach(), t0))
    assert changed > 0 and next(fus.momentum_scheduler) == 0.9 + 4 * (1.0 - 0.9) / 15


def _plain_steps(model, opt, x, first, count):
    for i in range(first, first + count):
        _backward(model, x, i)
        opt.step()
        opt.zero_grad()
        model.on_train_batch_end(None, x, i)


def test_state_dict_round_trip_continues_bit_identically():
    model, x = _step_module(partial(m3l_amd.DinoAdamW, lr=5e-4, weight_decay=0.05, max_grad_norm=1.0))
    opt, _, _ = model.configure_optimizers(5, 3)
    opt.bind_teacher(model)
    _plain_steps(model, opt, x, 0, 2)
    sd = copy.deepcopy(opt.state_dict())
    twin = copy.deepcopy(model)
    opt2, _, _ = twin.configure_optimizers(5, 3)
    opt2.bind_teacher(twin)
    opt2.param_groups[0]["lr"] = 123.0                 # must come back from the state dict
    opt2.load_state_dict(sd)
    assert opt2.step_count == 2 and opt2.param_groups[0]["lr"] == 5e-4 and opt2.param_groups[1]["WD_exclude"] is True
    _plain_steps(model, opt, x, 2, 1)
    _plain_steps(twin, opt2, x, 2, 1)
    for (k, a), (_, b) in zip(model.named_parameters(), twin.named_parameters()):
        assert torch.equal(a.detach(), b.detach()), k
    assert torch.equal(opt.exp_avg, opt2.exp_avg) and torch.equal(opt.exp_avg_sq, opt2.exp_avg_sq) and float(opt.exp_avg.abs().max()) > 0
    assert opt.step_count == opt2.step_count == 3


def test_sync_layout_gives_the_bits_of_the_own_layout():
    """sync=GradSync(model) at world size 1, no clipping: the parameters after 2 steps are bit-identical to the run on the optimizer's own
    buffers — the update is element-wise, only the layout differs."""
    own, x = _step_module(partial(m3l_amd.DinoAdamW, lr=5e-4, weight_decay=0.05))
    opt_o, _, _ = own.configure_optimizers(5, 3)
    shared, _ = _step_module(None)
    sync = GradSync(shared)
    shared.optim_partial = partial(m3l_amd.DinoAdamW, lr=5e-4, weight_decay=0.05, sync=sync)
    opt_s, _, _ = shared.configure_optimizers(5, 3)
    assert opt_s.flat is sync.flat and opt_s.flat_params is sync.flat_params
    assert [opt_s._span[id(p)] for p in opt_s._params] != [opt_o._span[id(p)] for p in opt_o._params]
    _plain_steps(own, opt_o, x, 0, 2)
    _plain_steps(shared, opt_s, x, 0, 2)
    for (k, a), (_, b) in zip(own.named_parameters(), shared.named_parameters()):
        assert torch.equal(a.detach(), b.detach()), k
    with pytest.raises(ValueError):
        m3l_amd.DinoAdamW([torch.nn.Parameter(torch.zeros(4, device=DEV))], sync=sync)
