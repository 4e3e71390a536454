"""`LatentTrainer` — drop-in for osu_dreamer/models/latent/train.py:35-255 on the HIP path.

Same constructor kwargs (the YAML keys under `model:` and the checkpoint's `hyper_parameters`), the same hooks and the same state-dict
layout (`latent.*`, `loss_ema`, `loss_ema_initialized`).  One step is `LatentModel`'s differentiable forward (latent_grad.py) with three
autograd nodes of this module around it, each a few launches of csrc/latent.hip and none of them a host read:

    z, s = encode_chart(chart)
    s_reg = od_mmd_imq(s, prior)                                   train.py:88      (_MMDFn: value and gradient in one pass)
    z', s', masked = od_latent_perturb(z, s, draws)                train.py:90-112  (_PerturbFn)
    logits, labels = latent(audio, z', s')
    loss, logs = od_latent_loss(logits, labels, chart, ...)        train.py:115-149 (_LossFn: sums, then one block that also keeps
                                                                                     loss_ema and its first-update flag on the device)

The optimizer is the reference's AdamW with Lightning's global-norm clip (optim.ClippedAdamW); there is no EMA model, parameter arena or
graph capture here.  The once-per-epoch validation metrics (train.py:176-255) are torch ops on the decoded maps, off the hot path;
`plot_val` (a TensorBoard figure) is not built.  Validation also takes whole maps in ragged groups (data.RaggedBeatmapBatch, from
`data.resident_val`): the varlen forward calls of LatentModel, then od_mmd_imq_pairs, od_latent_loss_maps and od_latent_eval_maps give every
map the values of its own per-map step, with one host read per group (`_validation_group`).
"""
from __future__ import annotations

import dataclasses
from typing import Any, Dict, List

import torch

from . import ops
from .data import RaggedBeatmapBatch
from .latent import LatentModel, LatentModelArgs
from .ldm import pad_to_multiple
from .lr_schedule import LRScheduleArgs, make_lr_schedule
from .optim import ClippedAdamW
from .train import HAVE_LIGHTNING, _Base

LOSS_COMPONENT_WEIGHTS = {          # train.py:21-33; od_latent_loss carries the same values
    "hit/onset": 1, "hit/combo": 1, "hit/slide": 1, "hit/sustain": 1, "hit/whistle": 1, "hit/finish": 1, "hit/clap": 1,
    "cursor/pos": 2, "cursor/vel": 2, "cursor/acc": 2, "label": 2,
}
LOG_NAMES = (*LOSS_COMPONENT_WEIGHTS, "s_reg", "loss")
ONSET, CURSOR = 0, slice(7, 9)      # data/beatmap/encode.py: BeatmapEncoding.ONSET, CursorSignals
F32 = torch.float32


def _plain_latent_args(latent_args) -> Dict[str, Any]:
    d = dataclasses.asdict(latent_args) if dataclasses.is_dataclass(latent_args) else dict(latent_args)
    if dataclasses.is_dataclass(d.get("ae_args")):
        d["ae_args"] = dataclasses.asdict(d["ae_args"])
    return d


def split_halves(x: torch.Tensor) -> torch.Tensor:
    """'b d (h l) -> (b h) d l', h = 2: each half of a window becomes a row of its own."""
    B, D, L2 = x.shape
    return x.reshape(B, D, 2, L2 // 2).permute(0, 2, 1, 3).reshape(2 * B, D, L2 // 2)


class _MMDFn(torch.autograd.Function):
    """s_reg = MMD^2(s, prior); its gradient is computed with the value and scaled by the incoming gradient in backward."""

    @staticmethod
    def forward(ctx, s, prior):
        s, prior = s.detach().to(F32).contiguous(), prior.detach().to(F32).contiguous()
        out = torch.empty(4, dtype=F32, device=s.device)
        ctx.ds = torch.empty_like(s)
        ops.mmd_imq(s, prior, out, ctx.ds, torch.empty(3 * s.shape[0], dtype=F32, device=s.device))
        return out[:1]

    @staticmethod
    def backward(ctx, g):
        ds = torch.empty_like(ctx.ds)
        ops.scale_by(ctx.ds, g.to(F32).contiguous(), ds)
        return ds, None


class _PerturbFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, z, s, draws, cfg, training):
        B2, E, l = z.shape
        dev = z.device
        z_out, s_out = torch.empty(B2, E, l, dtype=F32, device=dev), torch.empty(B2, s.shape[1], dtype=F32, device=dev)
        masked, span = torch.empty(B2, dtype=torch.uint8, device=dev), torch.empty(2 * B2, dtype=torch.int32, device=dev)
        ops.latent_perturb(z.detach().to(F32), s.detach().to(F32).contiguous(), *draws, z_out, s_out, masked, span, *cfg, training)
        ctx.masked, ctx.span = masked, span
        ctx.mark_non_differentiable(masked)
        return z_out, s_out, masked

    @staticmethod
    def backward(ctx, dz_out, ds_out, _):
        dz, ds = torch.empty_like(dz_out, dtype=F32), torch.empty_like(ds_out, dtype=F32)
        ops.latent_perturb_bwd(dz_out.to(F32).contiguous(), ds_out.to(F32).contiguous(), ctx.masked, ctx.span, dz, ds)
        return dz, ds, None, None, None


class _LossFn(torch.autograd.Function):
    """(loss, the 13 logged values).  When training, forward also updates loss_ema and its flag on the device."""

    @staticmethod
    def forward(ctx, logits, pred_labels, s_reg, chart, labels, masked, loss_ema, ema_flag, s_reg_weight, training):
        logits, pred_labels = logits.detach().to(F32).contiguous(), pred_labels.detach().to(F32).contiguous()
        B2, _, L = logits.shape
        dev = logits.device
        out, coef = torch.empty(13, dtype=F32, device=dev), torch.empty(11, dtype=F32, device=dev)
        ws = torch.empty(ops.latent_loss_ws_floats(B2, L), dtype=F32, device=dev)
        ops.latent_loss(logits, chart, pred_labels, labels, masked, s_reg.detach(), loss_ema, ema_flag, out, coef, ws, s_reg_weight, training)
        ctx.keep = (logits, chart, pred_labels, labels, masked, coef, s_reg_weight)
        ctx.mark_non_differentiable(out)
        return out[12:].clone(), out

    @staticmethod
    def backward(ctx, g, _):
        logits, chart, pred_labels, labels, masked, coef, w = ctx.keep
        dlogits, dlabels = torch.empty_like(logits), torch.empty_like(pred_labels)
        ds_reg = torch.empty(1, dtype=F32, device=logits.device)
        ops.latent_loss_bwd(logits, chart, pred_labels, labels, masked, coef, g.to(F32).contiguous(), dlogits, dlabels, ds_reg, w)
        return dlogits, dlabels, ds_reg, None, None, None, None, None, None, None


class LatentTrainer(_Base):
    validates_by_epoch = True       # fit.Trainer: validation = on_validation_epoch_start / validation_step / on_validation_epoch_end

    def __init__(
        self,
        # training parameters
        opt_args: Dict[str, Any],
        schedule_args: LRScheduleArgs,
        s_reg_weight: float,
        s_noise: float,
        z_noise: float,
        s_mask_frac: float,
        z_mask_frac: float,
        # model hparams
        emb_dim: int,
        style_dim: int,
        n_downs: int,
        stride: int,
        latent_args: LatentModelArgs,
    ):
        super().__init__()
        if HAVE_LIGHTNING:
            self.save_hyperparameters()
        self.hparams_dict = dict(opt_args=opt_args, schedule_args=schedule_args, s_reg_weight=s_reg_weight, s_noise=s_noise, z_noise=z_noise,
                                 s_mask_frac=s_mask_frac, z_mask_frac=z_mask_frac, emb_dim=emb_dim, style_dim=style_dim, n_downs=n_downs,
                                 stride=stride, latent_args=_plain_latent_args(latent_args))
        self.opt_args = dict(opt_args)
        self.lr_schedule = make_lr_schedule(schedule_args)
        self.s_reg_weight, self.s_noise, self.z_noise = float(s_reg_weight), float(s_noise), float(z_noise)
        self.s_mask_frac, self.z_mask_frac = float(s_mask_frac), float(z_mask_frac)
        self.register_buffer("loss_ema", torch.ones(len(LOSS_COMPONENT_WEIGHTS)))
        self.register_buffer("loss_ema_initialized", torch.tensor(False))
        self.latent = LatentModel(emb_dim, style_dim, n_downs, stride, LatentModelArgs(**_plain_latent_args(latent_args)))
        self.latent.requires_grad_(True)
        self.gradient_clip_val = None                      # set by the trainer shell (latent.yml)
        self._logged: Dict[str, torch.Tensor] = {}
        self._val: List[Dict[str, torch.Tensor]] = []

    # ------------------------------------------------------------------ loss (latent/train.py:75-154)
    def forward(self, batch, *, prior=None, eps_s=None, eps_z=None, u_s=None, repl=None, u_span=None, u_start=None):
        """(loss, logs) of one batch (audio (B, 72, 2L), chart (B, 9, 2L), labels (B, 5)), L a multiple of chunk_size.  The keywords pin
        the random draws for parity tests; by default they are drawn in the reference's order: the MMD prior, then, in training mode,
        eps_s, eps_z, u_s and repl (s_mask_frac > 0), u_span and u_start (z_mask_frac > 0)."""
        audio, chart, labels = batch
        audio, chart = split_halves(audio.to(F32)), split_halves(chart.to(F32)).contiguous()
        labels = labels.to(F32).repeat_interleave(2, dim=0).contiguous()
        z, s = self.latent.encode_chart(chart)
        B2, dev = s.shape[0], s.device
        on = lambda t: t.to(dev, F32).contiguous()
        prior = torch.randn_like(s) if prior is None else on(prior)
        s_reg = _MMDFn.apply(s, prior)
        draws = (None,) * 6
        if self.training:
            eps_s = torch.randn_like(s) if eps_s is None else on(eps_s)
            eps_z = torch.randn_like(z) if eps_z is None else on(eps_z)
            if self.s_mask_frac > 0:
                u_s = torch.rand(B2, device=dev) if u_s is None else on(u_s)
                repl = torch.randn_like(s) if repl is None else on(repl)
            if self.z_mask_frac > 0:
                u_span = torch.rand(B2, device=dev) if u_span is None else on(u_span)
                u_start = torch.rand(B2, device=dev) if u_start is None else on(u_start)
            draws = (eps_z, eps_s, u_s, repl, u_span, u_start)
        cfg = (self.s_noise, self.z_noise, self.s_mask_frac, self.z_mask_frac)
        z_in, s_in, masked = _PerturbFn.apply(z, s, draws, cfg, self.training)
        logits, pred_labels = self.latent(audio, z_in, s_in)
        loss, out = _LossFn.apply(logits, pred_labels, s_reg, chart, labels, masked, self.loss_ema,
                                  self.loss_ema_initialized.view(torch.uint8), self.s_reg_weight, self.training)
        return loss[0], {name: out[i] for i, name in enumerate(LOG_NAMES)}

    # ------------------------------------------------------------------ Lightning protocol
    def configure_optimizers(self):
        opt = ClippedAdamW(self.latent.parameters(), max_grad_norm=self.gradient_clip_val, **self.opt_args)
        return {
            "optimizer": opt,
            "lr_scheduler": {
                "scheduler": torch.optim.lr_scheduler.LambdaLR(opt, self.lr_schedule),
                "interval": "step",
            },
        }

    def _log(self, d: Dict[str, torch.Tensor]):
        self._logged.update(d)
        if HAVE_LIGHTNING and getattr(self, "_trainer", None) is not None:
            self.log_dict(d)

    def pad_batch(self, batch):
        """on_after_batch_transfer (train.py:165-169): both halves of a window must be chunk-aligned."""
        c = 2 * self.latent.chunk_size
        audio, chart, labels = batch
        return pad_to_multiple(audio, c), pad_to_multiple(chart, c), labels

    def training_step(self, batch, batch_idx, **pins):
        loss, log_dict = self(self.pad_batch(batch), **pins)
        self._log({f"train/{k}": v for k, v in log_dict.items()})
        return loss

    def on_train_batch_end(self, *args, **kwargs):
        pass

    def on_validation_epoch_start(self):
        self._on_pt = self._on_pp = self._on_tt = 0.        # onset soft-Dice sums
        self._cur_res = self._cur_tot = 0.                  # cursor R^2 sums: residual and total
        self._val = []

    @torch.no_grad()
    def validation_step(self, batch, batch_idx, *args, **pins):
        if isinstance(batch, RaggedBeatmapBatch):
            return self._validation_group(batch, **pins)
        batch = self.pad_batch(batch)
        _, log_dict = self(batch, **pins)
        logs = {f"val/{k}": v for k, v in log_dict.items()}
        logs.update(self.eval_metrics(batch))
        self._val.append(logs)
        return logs

    def _validation_group(self, b: RaggedBeatmapBatch, prior=None) -> List[Dict[str, torch.Tensor]]:
        """validation_step on G whole maps at once (data.RaggedBeatmapBatch): what the per-map step computes for each of them, by the
        varlen forward calls and the per-map reductions of csrc/latent.hip, with one device-to-host read for the group.

        Loss part, on the halves (map g = rows 2g, 2g + 1, as split_halves orders them): encode_chart, the MMD of each pair against its
        rows of one prior draw (2G, S) (`prior=` pins it), the eval-mode perturbation (each half decoded with the other half's style),
        audio_encoder, decode_logits, the label predictor and od_latent_loss_maps.  Metric part, on the whole maps: encode_chart, decode
        and od_latent_eval_maps.  `_val` receives one entry per map, in the group's order, and the five epoch sums grow in fp64 in that
        order."""
        c, m, dev = self.latent.chunk_size, self.latent, b.chart.device
        L = [int(x) for x in b.lengths]
        G, P = len(L), [(x + 2 * c - 1) // (2 * c) * (2 * c) for x in L]
        if tuple(b.chart.shape) != (G, 9, max(P)) or tuple(b.chart_halves.shape) != (2 * G, 9, max(P) // 2) or min(L) < 2 * c:
            raise ValueError(f"the group's maps ({L} frames) padded to multiples of 2 x chunk_size = {2 * c} do not give its tensors "
                             f"{tuple(b.chart.shape)} / {tuple(b.chart_halves.shape)}: the feed's pad multiple must be 2 x chunk_size")
        hl = [p // 2 for p in P for _ in range(2)]
        lens = m._dev_i32([hl, P + [0] * G, [p // c for p in P] + [0] * G], dev)
        hlens, plens, zlens = lens[0], lens[1, :G], lens[2, :G]
        labels = b.labels.to(F32).contiguous()
        # ---- the loss of every map's two halves
        chart_h = b.chart_halves.to(F32).contiguous()
        z, s = m.encode_chart(chart_h, lengths=hl)
        prior = torch.randn_like(s) if prior is None else prior.to(dev, F32).contiguous()
        out = torch.empty(G * (4 + 13 + 8), dtype=F32, device=dev)
        mmd, loss, ev = out[:4 * G].view(G, 4), out[4 * G:17 * G].view(G, 13), out[17 * G:].view(G, 8)
        ops.mmd_imq_pairs(s, prior, mmd, torch.empty(6 * G, dtype=F32, device=dev))
        cfg = (self.s_noise, self.z_noise, self.s_mask_frac, self.z_mask_frac)
        z_in, s_in, _ = _PerturbFn.apply(z, s, (None,) * 6, cfg, False)
        skips, _ = m.audio_encoder(b.audio_halves, lengths=hl)
        logits = m.decode_logits(z_in, s_in, skips=skips, lengths=hl)
        ws = torch.empty(ops.latent_loss_ws_floats(2 * G, chart_h.shape[-1]), dtype=F32, device=dev)
        ops.latent_loss_maps(logits, chart_h, hlens, m._label_predictor(s_in), labels.repeat_interleave(2, dim=0).contiguous(), mmd[:, 0],
                             self.loss_ema, loss, ws, self.s_reg_weight)
        # ---- the metrics of every whole map
        chart = b.chart.to(F32).contiguous()
        z, s = m.encode_chart(chart, lengths=P)
        pred_chart, pred_labels = m.decode(z, s, audio=b.audio, lengths=P)
        ws = torch.empty(ops.latent_eval_maps_ws_floats(G, chart.shape[-1]), dtype=F32, device=dev)
        ops.latent_eval_maps(chart, pred_chart, plens, z, zlens, pred_labels, labels, ev, ws)
        sums = ev[:, :5].cpu().double()                         # the group's one read; the logged values stay on the device
        logs = []
        for g in range(G):
            d = {f"val/{k}": loss[g, i] for i, k in enumerate(LOG_NAMES)}
            d.update({"eval/cursor_px_mae": ev[g, 5], "eval/label_mae": ev[g, 6], "eval/z_var_min": ev[g, 7]})
            tt, pt, pp, res, tot = sums[g].tolist()
            self._on_tt += tt
            self._on_pt += pt
            self._on_pp += pp
            self._cur_res += res
            self._cur_tot += tot
            logs.append(d)
        self._val.extend(logs)
        return logs

    def on_validation_epoch_end(self):
        """The batch means of every value validation_step logged, and the epoch sums' scores (train.py:191-208)."""
        def hmean(a, b):
            return 2 * a * b / max(a + b, 1e-8)

        logs = {k: torch.stack([d[k].detach().double() for d in self._val]).mean() for k in (self._val[0] if self._val else ())}
        onset_f1 = 2 * self._on_pt / max(self._on_pp + self._on_tt, 1e-8)
        cursor_q = self._cur_tot / max(self._cur_tot + self._cur_res, 1e-8)
        logs.update({"eval/hit/dice": onset_f1, "eval/cursor/vel/r2": 1. - self._cur_res / max(self._cur_tot, 1e-8),
                     "eval/score": hmean(onset_f1, cursor_q)})
        self._log(logs)
        return logs

    @torch.no_grad()
    def eval_metrics(self, b) -> Dict[str, torch.Tensor]:
        """train.py:210-255, for batch size 1 (full-length maps): plain torch ops on the decoded chart."""
        a, x, true_labels = b
        x, true_labels = x.to(F32), true_labels.to(F32)
        z, s = self.latent.encode_chart(x)
        pred_chart, pred_labels = self.latent.decode(z, s, audio=a)
        z_var_min = z.var(dim=(0, 2)).min()
        t, p = x[:, ONSET].float(), pred_chart[:, ONSET].float()
        self._on_tt += t.mul(t).sum().item()
        self._on_pt += p.mul(t).sum().item()
        self._on_pp += p.mul(p).sum().item()
        scale = x.new_tensor([512., 384.])[None, :, None]
        true_xy, pred_xy = x[:, CURSOR].float() * scale, pred_chart[:, CURSOR].float() * scale
        true_v, pred_v = true_xy.diff(dim=-1), pred_xy.diff(dim=-1)
        self._cur_res += (pred_v - true_v).pow(2).sum().item()
        self._cur_tot += (true_v - true_v.mean(dim=-1, keepdim=True)).pow(2).sum().item()
        return {"eval/cursor_px_mae": (pred_xy - true_xy).abs().mean(), "eval/label_mae": (pred_labels - true_labels).abs().mean(),
                "eval/z_var_min": z_var_min}
