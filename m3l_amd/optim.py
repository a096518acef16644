"""The optimizer side of a DINO iteration on the flat path: `DinoAdamW` and the two schedulers that drive it.

What the reference's trainer does after every backward (tactile_ssl/trainer/trainer.py:305-342) — clip_gradients(max_norm), AdamW over two
parameter groups (matrices decayed, vectors `WD_exclude`), the teacher's moving average, the lr and the wd scheduler — is here two
reduction launches plus ONE update launch (m3l_dino_opt_step, csrc/elementwise.hip) over flat parameter / gradient / moment / teacher
buffers.  The groups' lr and weight decay travel by value with the launch, so the schedulers cost nothing on the device.

`DinoAdamW` is a `torch.optim.Optimizer`: `partial(DinoAdamW, lr=..., weight_decay=...)` is a VTDINO `optim_cfg`, LRScheduler subclasses accept
it, and `param_groups` carries `lr`, `weight_decay`, `WD_exclude`, `initial_lr` as torch's does.  `WarmupCosineScheduler` and
`CosineWDSchedule` are the reference's schedulers (tactile_ssl/model/custom_scheduler.py: same signatures, same double arithmetic).
"""
import ctypes as C
import math
import weakref

import torch
from torch.optim.lr_scheduler import LRScheduler

MAX_GROUPS = 8          # DOPT_MAX_GROUPS of csrc/elementwise.hip


def build_segments(spans, n):
    """The segment tables of m3l_dino_opt_step.  spans: (start, end, group) per parameter, group = its hyper-parameter group or -1 for a
    parameter the update must leave alone; they must not overlap, stretches of [0, n) that no span covers become group -1.  Adjacent
    stretches of one group merge.  -> (seg_start, seg_group): seg_start has one entry more, ascends from 0 to n."""
    if n < 1:
        raise ValueError(f"build_segments: n = {n}")
    starts, groups, at = [], [], 0

    def put(a, b, g):
        if b <= a:
            return
        if groups and groups[-1] == g:
            return
        starts.append(a)
        groups.append(g)
    for a, b, g in sorted(spans):
        if a < at or b < a or b > n:
            raise ValueError(f"build_segments: span ({a}, {b}) overlaps its neighbour or leaves [0, {n})")
        put(at, a, -1)
        put(a, b, int(g))
        at = max(at, b)
    put(at, n, -1)
    return starts + [n], groups


class DinoAdamW(torch.optim.Optimizer):
    """torch.optim.AdamW(groups, lr, betas, eps, weight_decay) + clip_grad_norm_(max_grad_norm) + the teacher's moving average, one update
    launch per step.

    The parameters are re-homed into one flat buffer, group-major, and every `.grad` becomes a view of a flat gradient buffer that the
    backward accumulates into; with `sync=GradSync(model)` the optimizer adopts that object's buffers and spans instead (one owner of the
    storage under data parallelism; a parameter outside the sync is an error), joins its collectives and folds its 1 / world into the
    launch, as FlatAdam does.  Build it after the model is on its device, and do not move the model afterwards.

    A parameter that received no gradient since zero_grad() (`DinoVTT.pos_embedding`, which the forward never uses) is left alone — neither
    decayed nor given moments — as torch.optim.AdamW skips `.grad is None`; the segment tables are rebuilt and uploaded only when that set
    changes.  [A parameter that receives gradients in some steps only keeps the global step count in its bias correction; torch counts its
    own steps.]  betas and eps are common to all groups (at most 8 groups).

    zero_grad() always clears the flat gradient buffer in place, whatever `set_to_none` says: torch's default would cut the views loose.
    After step(), `last_grad_norm` is a device scalar with the norm clip_grad_norm_ would have returned (max_grad_norm=None: no clipping,
    the scalar stays 0); the clipped gradients are left in `.grad`.

    bind_teacher(model): from then on step() also applies `teacher = teacher * beta + (1 - beta) * student` in the same launch, beta drawn
    from the model inside step(); the model's on_train_batch_end then skips its own draw and update for that batch.
    """

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2, max_grad_norm=None, sync=None):
        if not 0.0 <= lr or not 0.0 <= eps or not 0.0 <= weight_decay or not (0.0 <= betas[0] < 1.0 and 0.0 <= betas[1] < 1.0):
            raise ValueError(f"DinoAdamW: lr={lr} betas={betas} eps={eps} weight_decay={weight_decay}")
        super().__init__(params, dict(lr=lr, betas=tuple(betas), eps=eps, weight_decay=weight_decay))
        if len(self.param_groups) > MAX_GROUPS:
            raise ValueError(f"DinoAdamW: {len(self.param_groups)} parameter groups, the update launch carries at most {MAX_GROUPS}")
        g0 = self.param_groups[0]
        for g in self.param_groups:
            if tuple(g["betas"]) != tuple(g0["betas"]) or g["eps"] != g0["eps"]:
                raise ValueError("DinoAdamW: betas and eps are common to all groups (only lr and weight_decay differ per group)")
        self.max_grad_norm = max_grad_norm
        self.sync = sync
        self.step_count = 0
        plist = [(k, p) for k, g in enumerate(self.param_groups) for p in g["params"]]
        if not plist:
            raise ValueError("DinoAdamW: no parameters")
        dev = plist[0][1].device
        for _, p in plist:
            if p.dtype != torch.float32 or p.device != dev or not p.is_contiguous():
                raise ValueError("DinoAdamW needs contiguous float32 parameters on one device")
        self._span, self._group_of = {}, {}
        if sync is not None:
            for k, p in plist:
                if id(p) not in sync._span:
                    raise ValueError(f"DinoAdamW(sync=...): a parameter of shape {tuple(p.shape)} is not part of the GradSync's flat buffer")
                self._span[id(p)] = sync._span[id(p)]
                self._group_of[id(p)] = k
            self.flat_params, self.flat = sync.flat_params, sync.flat
        else:
            total = sum(p.numel() for _, p in plist)
            self.flat_params = torch.empty(total, dtype=torch.float32, device=dev)
            self.flat = torch.zeros(total, dtype=torch.float32, device=dev)
            off = 0
            for k, p in plist:                       # group-major: a group's parameters are neighbours and merge into one segment
                n = p.numel()
                with torch.no_grad():
                    self.flat_params[off:off + n].copy_(p.detach().reshape(-1))
                    p.data = self.flat_params[off:off + n].view_as(p)
                p.grad = self.flat[off:off + n].view_as(p)
                self._span[id(p)] = (off, off + n)
                self._group_of[id(p)] = k
                off += n
        self._params = [p for _, p in plist]
        self._grad_views = [p.grad for p in self._params]
        self.exp_avg = torch.zeros_like(self.flat)
        self.exp_avg_sq = torch.zeros_like(self.flat)
        self._norm_ws = torch.zeros(1026, dtype=torch.float32, device=dev)
        self.last_grad_norm = self._norm_ws[1025]
        self._written = set()                    # id(param) that received a gradient since zero_grad() (as GradSync._written)
        me = weakref.ref(self)                   # (weak: the hooks outlive this object on the parameters)

        def _mark(q, _me=me):
            s = _me()
            if s is not None:
                s._written.add(id(q))
        self._hooks = [p.register_post_accumulate_grad_hook(_mark) for p in self._params]
        self._tables = {}                        # frozenset of active ids -> (seg_start, seg_group) on the device
        self._teacher_flat = None
        self._teacher_model = None
        self.last_ema_beta = None

    def __del__(self):
        for h in getattr(self, "_hooks", ()):
            try:
                h.remove()
            except Exception:      # noqa: BLE001  (interpreter shutdown)
                pass

    # ---- segment tables -----------------------------------------------------------------------------------------------------------------
    def _active(self):
        if self.sync is not None and self.sync._written:          # gradients a backward wrote straight into the sync's buffer
            return frozenset(self._written | (self.sync._written & self._span.keys()))
        return frozenset(self._written)

    def segment_spans(self, active):
        """(start, end, group or -1) per parameter for the set `active` of parameter ids: what build_segments takes."""
        return [(*self._span[id(p)], self._group_of[id(p)] if id(p) in active else -1) for p in self._params]

    def _tables_for(self, active):
        t = self._tables.get(active)
        if t is None:
            if len(self._tables) >= 8:
                self._tables.clear()
            starts, groups = build_segments(self.segment_spans(active), self.flat.numel())
            dev = self.flat.device
            t = (torch.tensor(starts, dtype=torch.int64, device=dev), torch.tensor(groups, dtype=torch.int32, device=dev))
            self._tables[active] = t
        return t

    # ---- the teacher ----------------------------------------------------------------------------------------------------------------------
    @torch.no_grad()
    def bind_teacher(self, model):
        """Pair model.student_encoder.parameters() with model.teacher_encoder.parameters() in order (the pairing of
        update_moving_average) and re-home the teacher's parameters into a flat buffer laid out like the student's: values and state-dict
        keys are unchanged.  `model` supplies the decay: next_moving_average_decay(), use_momentum."""
        for name in ("student_encoder", "teacher_encoder", "next_moving_average_decay"):
            if not hasattr(model, name):
                raise TypeError(f"DinoAdamW.bind_teacher: the model has no `{name}`")
        teacher = self.flat_params.clone()           # stretches without a pair average the student's own value with itself
        pairs = list(zip(model.student_encoder.parameters(), model.teacher_encoder.parameters()))
        for cur, ma in pairs:
            if id(cur) not in self._span:
                raise ValueError(f"DinoAdamW.bind_teacher: a student parameter of shape {tuple(cur.shape)} is not in this optimizer: the fused "
                                 "moving average covers the optimizer's parameters only")
            if cur.shape != ma.shape or ma.dtype != torch.float32 or ma.device != self.flat.device or not ma.is_contiguous():
                raise ValueError(f"DinoAdamW.bind_teacher: teacher parameter {tuple(ma.shape)} does not match its student {tuple(cur.shape)} "
                                 "(contiguous float32 on the optimizer's device expected)")
        for cur, ma in pairs:
            a, b = self._span[id(cur)]
            teacher[a:b].copy_(ma.detach().reshape(-1))
            ma.data = teacher[a:b].view_as(ma)
        self._teacher_flat = teacher
        self._teacher_model = model
        return self

    # ---- the step -------------------------------------------------------------------------------------------------------------------------
    def zero_grad(self, set_to_none: bool = False):
        """Always in place: the `.grad` views stay attached to the flat buffer (set_to_none is accepted and ignored)."""
        if self.sync is not None:
            self.sync.zero_grad()
        else:
            self.flat.zero_()
        self._written = set()

    @torch.no_grad()
    def step(self, closure=None):
        from . import _lib as L
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        if self.flat.device.type != "cuda":
            raise L.M3LError("DinoAdamW.step: the update is a HIP kernel, the parameters must live on a GPU (there is no CPU fallback)")
        for p, view in zip(self._params, self._grad_views):
            if p.grad is not view:
                raise RuntimeError("DinoAdamW.step: a parameter's .grad is no longer the view of the flat gradient buffer it was given "
                                   "(cleared with set_to_none outside optimizer.zero_grad(), or replaced)")
        gscale = 1.0
        if self.sync is not None:
            if self.sync._keep or self.sync._unscaled:     # a backward whose side-stream work / collectives have not been joined yet
                self.sync.finish(defer_scale=True)
            gscale = self.sync.take_scale()
        active = self._active()
        groups = self.param_groups
        n_groups = len(groups)
        g0 = groups[0]
        if active:                                   # (torch: a step in which no parameter has a gradient counts for none of them)
            self.step_count += 1
        seg_start, seg_group = self._tables_for(active)
        lr = (C.c_float * n_groups)(*[g["lr"] for g in groups])
        wd = (C.c_float * n_groups)(*[g["weight_decay"] for g in groups])
        teacher, beta = None, 0.0
        model = self._teacher_model
        if model is not None and model.use_momentum:
            beta = float(model.next_moving_average_decay())
            model._ema_in_step = True                # on_train_batch_end: the average of this batch is done
            self.last_ema_beta = beta
            teacher = self._teacher_flat.data_ptr()
        mx = float(self.max_grad_norm) if self.max_grad_norm is not None else 0.0
        L.check(L.lib().m3l_dino_opt_step(self.flat_params.data_ptr(), self.flat.data_ptr(), self.exp_avg.data_ptr(), self.exp_avg_sq.data_ptr(),
                                          teacher, self.flat.numel(), seg_start.data_ptr(), seg_group.data_ptr(), seg_group.numel(), lr, wd,
                                          n_groups, g0["betas"][0], g0["betas"][1], g0["eps"], max(self.step_count, 1), gscale, mx,
                                          self._norm_ws.data_ptr(), 1, beta, torch.cuda.current_stream().cuda_stream), "m3l_dino_opt_step")
        return loss

    # ---- checkpoints ----------------------------------------------------------------------------------------------------------------------
    def state_dict(self):
        """torch's layout — per parameter `step`, `exp_avg`, `exp_avg_sq` (copies, in the parameter's shape), and the groups with their
        hyper-parameters — so the file does not depend on how the flat buffer is laid out."""
        self.state.clear()
        for p in self._params:
            a, b = self._span[id(p)]
            self.state[p] = {"step": torch.tensor(float(self.step_count)), "exp_avg": self.exp_avg[a:b].view_as(p).clone(),
                             "exp_avg_sq": self.exp_avg_sq[a:b].view_as(p).clone()}
        sd = super().state_dict()
        self.state.clear()
        return sd

    @torch.no_grad()
    def load_state_dict(self, state_dict):
        super().load_state_dict(state_dict)
        steps = [0]
        for p in self._params:
            st = self.state.get(p)
            if not st:
                continue
            a, b = self._span[id(p)]
            self.exp_avg[a:b].copy_(st["exp_avg"].reshape(-1))
            self.exp_avg_sq[a:b].copy_(st["exp_avg_sq"].reshape(-1))
            steps.append(int(st["step"]))
        self.step_count = max(steps)
        self.state.clear()
        if len(self.param_groups) > MAX_GROUPS:
            raise ValueError(f"DinoAdamW: {len(self.param_groups)} parameter groups, at most {MAX_GROUPS}")


class WarmupCosineScheduler(LRScheduler):
    """Linear warm-up from start_lr to each group's base lr over warmup_epochs * steps_per_epoch steps, then half a cosine from the base lr
    down to final_lr over the remaining T_max - warm-up steps, never below final_lr.  The cosine is not stopped at T_max: as in the
    reference, a step past it climbs again.  The step it evaluates is the scheduler's call counter (`_step_count`: 1 after construction)."""

    def __init__(self, optimizer, steps_per_epoch, start_lr, T_max, warmup_epochs=10, last_epoch=-1, final_lr=0.0):
        self.start_lr = start_lr
        self.final_lr = final_lr
        self.warmup_steps = warmup_epochs * steps_per_epoch
        self.T_max = T_max - self.warmup_steps
        super().__init__(optimizer, last_epoch)

    def get_lr(self):
        t = self._step_count
        if t < self.warmup_steps:
            frac = float(t) / float(max(1, self.warmup_steps))
            return [self.start_lr + frac * (base - self.start_lr) for base in self.base_lrs]
        frac = float(t - self.warmup_steps) / float(max(1, self.T_max))
        half_cos = 1.0 + math.cos(math.pi * frac)
        return [max(self.final_lr, self.final_lr + (base - self.final_lr) * 0.5 * half_cos) for base in self.base_lrs]


class CosineWDSchedule:
    """Weight decay along half a cosine from ref_weight_decay to final_weight_decay over T_max steps, clamped at final_weight_decay on the
    side it approaches from (the cosine is not stopped at T_max: as in the reference, a step past it turns back); written into every group
    that is not marked `WD_exclude`.  step() returns the new value."""

    def __init__(self, optimizer, ref_weight_decay, T_max, final_weight_decay=0.0):
        self.optimizer = optimizer
        self.ref_weight_decay = ref_weight_decay
        self.final_weight_decay = final_weight_decay
        self.T_max = T_max
        self._step = 0.0

    def step(self):
        self._step += 1
        frac = self._step / self.T_max
        lo, hi = self.final_weight_decay, self.ref_weight_decay
        wd = lo + (hi - lo) * 0.5 * (1.0 + math.cos(math.pi * frac))
        wd = max(lo, wd) if lo <= hi else min(lo, wd)
        for group in self.optimizer.param_groups:
            if not group.get("WD_exclude", False):
                group["weight_decay"] = wd
        return wd
