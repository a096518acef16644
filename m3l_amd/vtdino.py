"""DINO self-distillation on top of the DINO-style encoder (`DinoVTT`) — drop-in for the reference's `models/vtdino.py` (VTDINO): same
constructor keywords, attributes, state-dict keys and training interface (`sample_masks`, `forward`, `training_step`,
`on_train_batch_end`, `configure_optimizers`, `teacher_temp_schedule`).

One step: the student encoder runs the global views and the local views (two passes, their token counts differ), the register token of
every view goes through the head's MLP and L2 normalisation in one batch of P x B rows, the teacher (no gradient) runs the global views,
and the prototype layer, the centred-teacher cross-entropy and their backward are one autograd node on the kernels of csrc/dino.hip
(m3l_amd/dino.py).  The block-mask sampler runs on the CPU with `self.generator` and returns the reference's indices bit for bit.

`centering="sinkhorn_knopp"` (a trailing keyword the reference's VTDINO does not have; its DINOv2 algorithm does) takes the Sinkhorn-Knopp
assignment of the teacher logits as the targets: DINOLoss.sinkhorn_knopp_center gives the K-vector that stands in the centre's place, and
the centre is neither applied nor updated.

`koleo_weight > 0` (another trailing keyword; the reference's DINOv2 algorithm has it, 0.1 there) adds the KoLeo regulariser of
`tactile_ssl/loss/koleo_loss.py` on the student's register rows of the global views: one group per global view, so samples of different
views are never compared, the views' losses summed, all in one set of launches (KoLeoFn).  At 0.0 the step is the one without it.

`ibot=True` (a trailing keyword; the third term of the reference's DINOv2 algorithm, `tactile_ssl/algorithm/dinov2.py`) adds the iBOT patch loss
`ibot_patch_loss(student patch logits, teacher patch targets) / num_global_masks`: the patch tokens of the student's global pass (the same
forward_features call that yields the register rows) go through `dino_head`'s MLP — or `ibot_head`'s with `ibot_separate_head=True`, a
fresh head in each of the student and teacher dicts — the teacher's global patch tokens through the teacher's, and the prototype layer, the
cross-entropy over the Q x (B n) patch rows and their backward are one autograd node, reached through the same `_head_loss` as the DINO
term's: IbotHeadLossFn, which is HeadLossFn on the row-tiled kernels (m3l_op_ibot_*).  The targets are centred (iBOTPatchLoss.center,
one-step delay) or Sinkhorn-Knopp over all patch rows, as `centering` says.  With the
defaults neither `ibot_patch_loss` nor `ibot_head` exists and the module, its state dict and its step are the ones without the keywords.

Not built: online probes and their logging (a non-empty `online_probes` is refused).
"""
import copy
import math
from functools import partial

import torch
from torch import nn

from . import functional as Fn
from .dino import DINOLoss, HeadLossFn, IbotHeadLossFn, KoLeoFn, KoLeoLoss, iBOTPatchLoss, update_moving_average


class VTDINO(nn.Module):
    def __init__(self, encoder, dino_head, optim_cfg, lr_scheduler_cfg, wd_scheduler_cfg, online_probes=None, online_probes_lrs=[],
                 local_mask_scale=(0.2, 0.8), global_mask_scale=(0.2, 0.8), num_global_masks=1, num_local_masks=4, min_keep_num_sensors=4,
                 allow_mask_overlap=False, moving_average_decay=0.99, teacher_temp=(0.04, 0.07), teacher_warmup_epochs=10, use_momentum=True,
                 log_freq_reconstruction=1000, centering="centering", koleo_weight=0.0, ibot=False, ibot_separate_head=False):
        super().__init__()
        for name, value in (("ibot", ibot), ("ibot_separate_head", ibot_separate_head)):
            if not isinstance(value, bool):
                raise ValueError(f"VTDINO({name}=...): True or False expected, got {value!r}")
        if ibot_separate_head and not ibot:
            raise ValueError("VTDINO(ibot_separate_head=True) needs ibot=True: without the patch loss nothing would use the head")
        self.ibot, self.ibot_separate_head = ibot, ibot_separate_head
        if not koleo_weight >= 0:
            raise ValueError(f"VTDINO(koleo_weight=...): a weight >= 0 expected, got {koleo_weight!r}")
        self.koleo_weight = float(koleo_weight)
        if centering not in ("centering", "sinkhorn_knopp"):
            raise ValueError(f"VTDINO(centering=...): 'centering' or 'sinkhorn_knopp' expected, got {centering!r}")
        self.centering = centering
        if online_probes:
            raise NotImplementedError("VTDINO(online_probes=...): online probes and their logging are not part of this package")
        assert len(online_probes_lrs) == 0, "Number of online probes should match the number of learning rates"
        self.optim_partial = optim_cfg
        self.lr_scheduler_partial = lr_scheduler_cfg
        self.wd_scheduler_partial = wd_scheduler_cfg
        self.use_momentum = use_momentum
        self.global_mask_scale = global_mask_scale
        self.local_mask_scale = local_mask_scale
        self.num_global_masks = num_global_masks
        self.num_local_masks = num_local_masks
        self.min_keep = min_keep_num_sensors
        self.allow_mask_overlap = allow_mask_overlap
        self.log_freq_img = log_freq_reconstruction
        self.generator = torch.Generator()
        self.step = -1

        self.compute_dtype = getattr(encoder, "compute_dtype", "fp32")
        dino_head = partial(dino_head, in_dim=encoder.embed_dim)
        self.student_encoder_dict, self.teacher_encoder_dict = dict(), dict()
        self.student_encoder_dict["backbone"] = encoder
        self.student_encoder_dict["dino_head"] = dino_head()
        if ibot_separate_head:
            self.student_encoder_dict["ibot_head"] = dino_head()
        self.student_encoder = nn.ModuleDict(self.student_encoder_dict)
        self.teacher_encoder_dict["backbone"] = copy.deepcopy(encoder)
        self.teacher_encoder_dict["dino_head"] = dino_head()          # a fresh head, not a copy of the student's
        if ibot_separate_head:
            self.teacher_encoder_dict["ibot_head"] = dino_head()
        self.teacher_encoder = nn.ModuleDict(self.teacher_encoder_dict)
        self.teacher_encoder.requires_grad_(False)
        for net in (self.student_encoder_dict, self.teacher_encoder_dict):
            for name in ("dino_head", "ibot_head"):
                if name in net:
                    net[name].compute_dtype = self.compute_dtype
        self.dino_loss = DINOLoss(out_dim=self.student_encoder_dict["dino_head"].last_layer.out_features)
        if ibot:
            self.ibot_patch_loss = iBOTPatchLoss(patch_out_dim=self.student_encoder_dict["dino_head"].last_layer.out_features)
        self.koleo_loss = KoLeoLoss()                              # no parameters, no buffers: the state dict is unchanged

        self.patch_size = encoder.image_patch_height
        self.img_size = encoder.image_height
        self.in_chans = encoder.image_channels
        self.online_probes = []
        self.online_probes_lrs = online_probes_lrs

        self.momentum_scheduler = None
        self._ema_in_step = False            # set by DinoAdamW.step() (bound teacher): this batch's moving average is already applied
        self.moving_average_decay =self._float_or_pair(moving_average_decay, "moving_average_decay")
        self.teacher_temp_scheduler = None
        self.teacher_temp = self._float_or_pair(teacher_temp, "teacher_temp")
        self.teacher_warmup_epochs = teacher_warmup_epochs
        self.val_reconstruction_error = []
        self.last = {}                       # student / teacher logits of the last forward (detached), for inspection
        self.loss_terms = None               # (DINO loss, weighted KoLeo loss) of the last forward when koleo_weight > 0
        self.loss_parts = None               # {name: term} of the last forward when it has more than the DINO term (ibot, koleo_weight > 0)

    @staticmethod
    def _float_or_pair(value, name):
        if isinstance(value, float):
            return value
        if isinstance(value, (str, bytes)) or not hasattr(value, "__len__"):
            raise TypeError(f"{name} must be a float or a sequence of two floats, got {value!r}")
        assert len(value) == 2, f"{name} needs two values (start, end)"
        return tuple(float(v) for v in value)

    # ---- block-mask sampler (CPU, self.generator) -----------------------------------------------------------------------------------
    def _sample_block_size(self, height, width, scale):
        r = torch.rand(1, generator=self.generator).item()
        lo, hi = scale
        max_keep = int(height * width * (lo + r * (hi - lo)))
        h = w = int(round(math.sqrt(max_keep)))            # aspect ratio 1
        h, w = min(h, height), min(w, width)
        if h * w <= self.min_keep:
            raise ValueError(f"mask scale {tuple(scale)} drew a {h}x{w} block on the {height}x{width} patch grid: a block is accepted only "
                             f"with more than min_keep_num_sensors = {self.min_keep} patches, so no placement of it can ever pass "
                             "(the sampler would retry for ever); raise the lower scale bound or lower min_keep_num_sensors")
        return h, w

    def _sample_block_mask(self, height, width, b_size, acceptable_regions=None):
        h, w = b_size
        tries, timeout = 0, 20
        while True:
            top = torch.randint(0, height - h + 1, (1,), generator=self.generator)
            left = torch.randint(0, width - w + 1, (1,), generator=self.generator)
            mask = torch.zeros((height, width), dtype=torch.int32)
            mask[top:top + h, left:left + w] = 1
            if acceptable_regions is not None:
                # all but the last `tries` regions still constrain the block
                for region in acceptable_regions[:max(len(acceptable_regions) - tries, 0)]:
                    mask *= region
            idx = torch.nonzero(mask.flatten())
            if len(idx) > self.min_keep:
                break
            timeout -= 1
            if timeout == 0:                               # 20 failures: drop one more acceptable region
                tries += 1
                timeout = 20
        complement = torch.ones((height, width), dtype=torch.int32)
        complement[top:top + h, left:left + w] = 0
        return idx.squeeze(), complement

    def _fast_blocks(self, count, height, width, b_size):
        """`count` unconstrained blocks: each is accepted at its first placement (its h * w patches exceed min_keep), so the generator
        only ever yields (top, left) pairs; with equal bounds for both they are drawn in one call, which consumes the generator exactly
        as the pairs drawn one by one do.  -> (count, h * w) patch indices in ascending order, as nonzero() lists them."""
        h, w = b_size
        n_top, n_left = height - h + 1, width - w + 1
        if n_top == n_left:
            tl = torch.randint(0, n_top, (2 * count,), generator=self.generator).view(count, 2)
            top, left = tl[:, 0], tl[:, 1]
        else:
            pairs = [(torch.randint(0, n_top, (1,), generator=self.generator), torch.randint(0, n_left, (1,), generator=self.generator))
                     for _ in range(count)]
            top, left = torch.cat([p[0] for p in pairs]), torch.cat([p[1] for p in pairs])
        rows = top[:, None] + torch.arange(h)[None, :]
        cols = left[:, None] + torch.arange(w)[None, :]
        return (rows[:, :, None] * width + cols[:, None, :]).reshape(count, h * w)

    def sample_masks(self, x):
        batch_size, _, image_height, image_width = x.shape
        height, width = image_height // self.patch_size, image_width // self.patch_size
        local_size = self._sample_block_size(height, width, self.local_mask_scale)
        global_size = self._sample_block_size(height, width, self.global_mask_scale)
        if self.allow_mask_overlap:
            # nothing constrains a block: per sample the local blocks, then the global ones, two generator calls each at most
            per_sample = [(self._fast_blocks(self.num_local_masks, height, width, local_size),
                           self._fast_blocks(self.num_global_masks, height, width, global_size)) for _ in range(batch_size)]
            local = torch.stack([s[0] for s in per_sample], dim=1).to(x.device)       # (masks, B, n)
            global_ = torch.stack([s[1] for s in per_sample], dim=1).to(x.device)
            return list(global_.unbind(0)), list(local.unbind(0))
        all_local, all_global = [], []
        keep_local = keep_global = height * width
        for _ in range(batch_size):
            locals_, complements = [], []
            for _ in range(self.num_local_masks):
                m, c = self._sample_block_mask(height, width, local_size)
                locals_.append(m)
                complements.append(c)
                keep_local = min(keep_local, len(m))
            all_local.append(locals_)
            globals_ = []
            for _ in range(self.num_global_masks):
                m, _c = self._sample_block_mask(height, width, global_size, complements)
                globals_.append(m)
                keep_global = min(keep_global, len(m))
            all_global.append(globals_)
        # every mask cut to the smallest of its kind, then one (B, n) index tensor per mask
        global_masks = [torch.stack([sample[i][:keep_global] for sample in all_global]).to(x.device) for i in range(self.num_global_masks)]
        local_masks = [torch.stack([sample[i][:keep_local] for sample in all_local]).to(x.device) for i in range(self.num_local_masks)]
        return global_masks, local_masks

    # ---- the step -------------------------------------------------------------------------------------------------------------------
    @staticmethod
    def _rows_and_patches(backbone, x, masks):
        out = backbone.forward_features(x, masks)
        assert "x_norm_regtokens" in out, "Dino requires backbone to contain 1 register token"
        reg = out["x_norm_regtokens"]
        assert reg.shape[1] == 1, f"VTDINO needs exactly one register token, the backbone has {reg.shape[1]}"
        return reg[:, 0], out["x_norm_patchtokens"]         # ((p b), c) and ((p b), n, c), view-major

    @classmethod
    def _register_rows(cls, backbone, x, masks):
        return cls._rows_and_patches(backbone, x, masks)[0]

    def forward(self, x, global_masks, local_masks):
        assert global_masks is not None and local_masks is not None, "Masks are required for DINOModule during training"
        student, teacher = self.student_encoder_dict, self.teacher_encoder_dict
        P, Q = len(global_masks) + len(local_masks), len(global_masks)
        global_rows, global_patches = self._rows_and_patches(student["backbone"], x, global_masks)
        rows = torch.cat([global_rows, self._register_rows(student["backbone"], x, local_masks)], dim=0)
        xn = student["dino_head"].normalized(rows)
        B = xn.shape[0] // P
        with torch.no_grad():
            t_rows, t_patches = self._rows_and_patches(teacher["backbone"], x, global_masks)
        loss = self._head_loss("dino_head", self.dino_loss, HeadLossFn, P, xn, t_rows, (Q, B), (Q, B), "teacher_logits")
        self.loss_terms = self.loss_parts = None
        terms = {"dino_loss": loss.detach()}
        if self.ibot:
            # patches ((q b), n, c) of the student's global views: R = B n rows of a view, r = b n + k; the centre's sums take ((q b), n, K)
            name = "ibot_head" if self.ibot_separate_head else "dino_head"
            QB, n, _ = global_patches.shape
            patch = self._head_loss(name, self.ibot_patch_loss, IbotHeadLossFn, Q, student[name].normalized(global_patches), t_patches,
                                    (Q, QB // Q * n), (QB, n), "teacher_patch_logits") / self.num_global_masks
            terms["ibot_loss"] = patch.detach()
            loss = loss + patch
        if self.koleo_weight > 0:
            # one group per global view (the rows are view-major); local to the rank under data parallelism, as in the reference
            keep = {}
            koleo = self.koleo_weight * KoLeoFn.apply(global_rows, Q, 1e-8, keep)
            self.last["koleo_indices"] = self.koleo_loss.last = keep["indices"]
            terms["koleo_loss"] = koleo.detach()
            self.loss_terms = (terms["dino_loss"], terms["koleo_loss"])
            loss = loss + koleo
        if len(terms) > 1:
            self.loss_parts = terms
        return loss

    def _head_loss(self, name, loss_mod, node, views, xn, t_in, paired, samples, last_key):
        """One cross-entropy term, unscaled: x_n (views x rows, D) of the student's head `name` against the teacher's head `name` on t_in (no
        gradient), in the head + loss node `node` of the term's kernel family.  `paired` = (Q, rows) is the shape in which the teacher
        logits meet the student's and are kept in self.last[last_key], `samples` the leading shape in which `loss_mod` takes them for its centre."""
        last_layer = self.student_encoder_dict[name].last_layer
        with torch.no_grad():
            t_logits = self.teacher_encoder_dict[name](t_in)
            if self.centering == "sinkhorn_knopp":      # over all rows; the targets' K-vector stands where the centre stands, the centre is never updated
                center = loss_mod.sinkhorn_knopp_center(t_logits, self.current_teacher_temp)
            else:
                loss_mod.apply_center_update()
                center = loss_mod.center
        t_paired = t_logits.view(*paired, -1)
        loss = node.apply(Fn.dtype_code(self.compute_dtype), views, xn, last_layer.weight_v, last_layer.weight_g, t_paired, center,
                                loss_mod.student_temp, self.current_teacher_temp, self.last)
        self.last[last_key] = t_paired
        if self.centering != "sinkhorn_knopp":
            loss_mod.update_center(t_logits.view(*samples, -1))
        return loss

    def training_step(self, batch, batch_idx):
        self.step = self.step + 1
        self.generator.manual_seed(self.step)
        global_masks, local_masks = self.sample_masks(batch["image"])
        loss = self.forward(batch, global_masks, local_masks)
        if self.loss_parts is None:
            output = {"ssl_loss": loss.item()}
        else:                                                # every scalar in one device-to-host copy
            names = list(self.loss_parts)
            values = torch.stack([loss.detach()] + [self.loss_parts[k] for k in names]).tolist()
            output = dict(zip(["ssl_loss"] + names, values))
        online_probes_loss = 0.0
        output["loss"] = loss
        output["online_probes_loss"] = online_probes_loss
        return output

    def validation_step(self, batch, batch_idx):
        return self.training_step(batch, batch_idx)

    def on_train_batch_end(self, outputs, batch, batch_idx, trainer_instance=None):
        assert self.teacher_encoder is not None, "target encoder has not been created"
        self.current_teacher_temp = next(self.teacher_temp_scheduler) if self.teacher_temp_scheduler is not None else self.teacher_temp
        if self._ema_in_step:      # a DinoAdamW with this model's teacher bound drew the decay and applied the average inside its step()
            self._ema_in_step = False
            return
        if self.use_momentum:
            update_moving_average(self.teacher_encoder, self.student_encoder, self.next_moving_average_decay())

    def next_moving_average_decay(self):
        """The teacher's decay for the next update: the next value of the schedule configure_optimizers() set up, or the constant.  Each
        call consumes one value (on_train_batch_end, or DinoAdamW.step() with a bound teacher — never both for one batch)."""
        return next(self.momentum_scheduler) if self.momentum_scheduler is not None else self.moving_average_decay

    def configure_optimizers(self, num_iterations_per_epoch, num_epochs):
        params = [p for pn, p in self.named_parameters() if not pn.startswith("online_probes") and p.requires_grad]
        optim_groups = [{"params": [p for p in params if p.dim() >= 2]},
                        {"params": [p for p in params if p.dim() < 2], "WD_exclude": True, "weight_decay": 0.0}]
        optimizer = self.optim_partial(optim_groups)
        if self.lr_scheduler_partial is None:
            return optimizer, None, None
        total = num_epochs * num_iterations_per_epoch
        lr_scheduler = self.lr_scheduler_partial(optimizer=optimizer, T_max=int(total), steps_per_epoch=num_iterations_per_epoch)
        if isinstance(self.moving_average_decay, tuple):
            d0, d1 = self.moving_average_decay
            self.momentum_scheduler = (d0 + i * (d1 - d0) / total for i in range(int(total) + 1))
        self.current_teacher_temp = self.teacher_temp
        if isinstance(self.teacher_temp, tuple):
            self.teacher_temp_scheduler = self.teacher_temp_schedule(num_epochs, num_iterations_per_epoch)
            self.current_teacher_temp = self.teacher_temp[0]
        lr_entry = {"scheduler": lr_scheduler, "interval": "step", "monitor": None}
        if self.wd_scheduler_partial is None:
            return optimizer, lr_entry, None
        wd_scheduler = self.wd_scheduler_partial(optimizer, T_max=int(total))
        return optimizer, lr_entry, {"wd_scheduler": wd_scheduler, "interval": "step", "frequency": 1}

    def teacher_temp_schedule(self, num_epochs, num_iterations_per_epoch):
        assert isinstance(self.teacher_temp, tuple), "Teacher temp must be a tuple if this function is called"
        t0, t1 = self.teacher_temp
        warm = self.teacher_warmup_epochs * num_iterations_per_epoch
        for i in range(int(num_epochs * num_iterations_per_epoch) + 1):
            yield t1 if i > warm else t0 + i * (t1 - t0) / warm
