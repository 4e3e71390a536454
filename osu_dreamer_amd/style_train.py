"""`StyleTrainer` — drop-in for osu_dreamer/models/style/train.py:18-160 on the HIP path.

Same constructor kwargs (the YAML keys under `model:` and the checkpoint's `hyper_parameters`), the same hooks and the same state-dict
layout (`style.*`, `style_ema.module.*`, `style_ema.n_averaged`).  The step is one autograd node: lerp + distance-marching loss
(od_make_xt / od_loss_grad / od_loss_finalize with E = style_dim, L = 1: `frame_dist_sq` over one frame is the plain channel sum of
train.py:69-84), `StyleModel.train_forward` and, on `loss.backward()`, `StyleModel.train_backward` straight into the arena's gradient
buffer.  The optimizer is `FusedAdamWEMA` over `self.style` alone (train.py:94), with the decay-0.99 average fused into its pass.

The once-per-epoch validation metrics (nearest-neighbour ratios, recall, spread, energy distance: train.py:120-160) are pairwise
distances over a few hundred rows, off the hot path: they are torch ops on the device tensors; the samples they measure come from the
EMA model's HIP `sample`.
"""
from __future__ import annotations

import dataclasses
from typing import Any, Dict, List, Optional

import torch
from torch import nn

from . import ops
from .lr_schedule import LRScheduleArgs, make_lr_schedule
from .optim import FusedAdamWEMA
from .style import StyleModel, StyleModelArgs
from .train import HAVE_LIGHTNING, _Base


class StyleEMAModel(nn.Module):
    """Stand-in for AveragedModel(style, multi_avg_fn=get_ema_multi_avg_fn(.99)) (style/train.py:46): `.module` is a frozen StyleModel
    holding the averaged weights (and the rff buffers), `n_averaged` a long buffer.  The average is produced by the fused optimizer pass;
    `update_parameters` outside that pass runs the same kernel in EMA-only form (first update copies, then lerp)."""

    def __init__(self, model: StyleModel, decay: float = 0.99):
        super().__init__()
        self.module = StyleModel(model.style_dim, model.args)
        self.module.load_state_dict(model.state_dict())
        self.module.requires_grad_(False)
        self.decay = decay
        self.register_buffer("n_averaged", torch.tensor(0, dtype=torch.long))
        self.fused_pending = 0
        self.count = 0            # host mirror of n_averaged (no device sync in the step)

    def update_parameters(self, model: StyleModel):
        if self.fused_pending > 0:          # already averaged inside the optimizer's pass
            self.fused_pending -= 1
        else:
            ops.ema_update(self.module.arena.data, model.arena.data, self.decay, 1 if self.count == 0 else 2)
        self.count += 1
        self.n_averaged += 1

    def _load_from_state_dict(self, state_dict, prefix, *args, **kwargs):
        super()._load_from_state_dict(state_dict, prefix, *args, **kwargs)
        if prefix + "n_averaged" in state_dict:
            self.count = int(state_dict[prefix + "n_averaged"])


def _plain_style_args(style_args) -> Dict[str, Any]:
    if isinstance(style_args, dict):
        return dict(style_args)
    return dataclasses.asdict(style_args)


class StyleTrainer(_Base):
    validates_by_epoch = True       # fit.Trainer: validation = on_validation_epoch_start / validation_step / on_validation_epoch_end

    def __init__(
        self,
        # training parameters
        opt_args: Dict[str, Any],
        schedule_args: LRScheduleArgs,
        label_drop_prob: float,
        osl_weight: float,
        del_weight: float,
        # model hparams
        style_dim: int,
        style_args: StyleModelArgs,
    ):
        super().__init__()
        if HAVE_LIGHTNING:
            self.save_hyperparameters()
        self.hparams_dict = dict(opt_args=opt_args, schedule_args=schedule_args, label_drop_prob=label_drop_prob, osl_weight=osl_weight,
                                 del_weight=del_weight, style_dim=style_dim, style_args=_plain_style_args(style_args))
        self.opt_args = dict(opt_args)
        self.lr_schedule = make_lr_schedule(schedule_args)
        self.label_drop_prob = float(label_drop_prob)
        self.osl_weight = float(osl_weight)
        self.del_weight = float(del_weight)
        self.style = StyleModel(style_dim, StyleModelArgs(**_plain_style_args(style_args)))
        self.style.requires_grad_(True)                     # only the trainer's own model is trainable
        self.style_ema = StyleEMAModel(self.style, decay=0.99)
        self.gradient_clip_val: Optional[float] = None      # set by the trainer shell (style.yml)
        # capture forward + loss + backward of the training step into one hipGraph (GPU only).  With it, the gradients are accumulated when
        # the loss is computed and `loss.backward()` takes the seed gradient as 1
        self.use_graph = True
        self._graph = _StepGraph()
        self._logged: Dict[str, torch.Tensor] = {}
        self._val_s: List[torch.Tensor] = []
        self._val_labels: List[torch.Tensor] = []

    # ------------------------------------------------------------------ loss (style/train.py:48-91)
    def forward(self, model: StyleModel, _h, _z, s1, labels, *, t=None, s0=None, drop=None):
        """Distance-marching loss on style codes.  `t` (B,), `s0` (B, S) and `drop` (B, 5, the uniform draws compared with
        label_drop_prob) pin the noise for parity tests; by default they are drawn in the reference's order (train.py:59-65)."""
        B, dev = s1.size(0), s1.device
        if t is None:
            u01 = (torch.randperm(B, device=dev) + torch.rand(B, device=dev)) / B
            t = torch.special.ndtri(u01.clamp(1e-6, 1 - 1e-6)).sigmoid().to(torch.float32)
        if s0 is None:
            s0 = torch.randn_like(s1, dtype=torch.float32)
        if drop is None:
            drop = torch.rand_like(labels, dtype=torch.float32)
        masked = torch.where(drop.to(dev) < self.label_drop_prob, -1.0, labels.to(torch.float32))
        needs_grad = torch.is_grad_enabled() and any(p.requires_grad for p in model.parameters())
        graph = self._graph if (needs_grad and self.use_graph and dev.type == "cuda" and model is self.style) else None
        out = _StyleLossFn.apply(model, self.osl_weight, self.del_weight, graph, s1, masked, t, s0, *(model.parameters() if needs_grad else ()))
        logs = {"loss": out[0].detach(), "osl": out[1].detach(), "del": out[2].detach(), "u_mape": out[3].detach()}
        return out[0], logs

    # ------------------------------------------------------------------ Lightning protocol
    def configure_optimizers(self):
        opt = FusedAdamWEMA(self.style, ema=self.style_ema, **self.opt_args)
        opt.max_grad_norm = self.gradient_clip_val
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

    def training_step(self, batch, batch_idx, **pins):
        loss, log_dict = self(self.style, *batch, **pins)
        self._log({f"train/{k}": v for k, v in log_dict.items()})
        return loss

    def on_train_batch_end(self, *args, **kwargs):
        self.style_ema.update_parameters(self.style)

    def on_validation_epoch_start(self):
        self._val_s, self._val_labels = [], []

    def validation_step(self, batch, batch_idx, *args, **kwargs):
        _, _, s, labels = batch
        self._val_s.append(s.detach())
        self._val_labels.append(labels.detach())

    def on_validation_epoch_end(self, *, t=None, s0=None, drop=None, s_init=None):
        """train.py:120-150.  `t` / `s0` / `drop` pin the loss draws and `s_init` (K tensors (B, S)) the samplers' starting noise."""
        s_real = torch.cat(self._val_s).to(torch.float32)
        labels = torch.cat(self._val_labels).to(torch.float32)
        B = s_real.size(0)
        ema = self.style_ema.module
        with torch.no_grad():
            _, log_dict = self(ema, None, None, s_real, labels, t=t, s0=s0, drop=drop)
        logs = {f"val/{k}": v for k, v in log_dict.items()}
        if B >= 2:
            K = 4
            samp = torch.stack([ema.sample(labels, 16, s_init=None if s_init is None else s_init[k]) for k in range(K)])   # K B S
            logs.update(sample_metrics(samp, s_real, labels))
        self._log(logs)
        return logs


def _nn_mean(a: torch.Tensor, b: torch.Tensor, exclude_self: bool = False) -> torch.Tensor:
    d = torch.cdist(a, b)
    if exclude_self:
        d = d.clone().fill_diagonal_(float("inf"))
    return d.min(1).values.mean()


def energy_distance(x: torch.Tensor, y: torch.Tensor) -> torch.Tensor:
    """2 E|x - y| - E|x - x'| - E|y - y'| with the self-pairs left out of the last two means (train.py:153-160)."""
    def within(a):
        n = a.size(0)
        return torch.cdist(a, a).sum() / (n * (n - 1))
    return 2 * torch.cdist(x, y).mean() - within(x) - within(y)


def sample_metrics(samp: torch.Tensor, s_real: torch.Tensor, labels: torch.Tensor) -> Dict[str, torch.Tensor]:
    """The five sample metrics of train.py:132-150 for samp (K, B, S) drawn under `labels` against the real codes s_real (B, S)."""
    K, B, _ = samp.shape
    out: Dict[str, torch.Tensor] = {}
    rr = _nn_mean(s_real, s_real, True)
    flat = samp.flatten(0, 1)
    out["val/nn_ratio"] = _nn_mean(flat, s_real) / rr
    hi = labels[:, 0] >= 5
    if int(hi.sum()) > 1:
        R = s_real[hi]
        out["val/nn_ratio_sr5"] = _nn_mean(samp[:, hi].flatten(0, 1), R) / _nn_mean(R, R, True)
    out["val/cond_recall"] = (samp - s_real[None]).norm(dim=-1).min(0).values.mean()
    per_cond = samp.transpose(0, 1)
    out["val/sample_spread"] = torch.cdist(per_cond, per_cond).sum() / (K * (K - 1) * B) / rr
    out["val/energy_dist"] = energy_distance(flat, s_real)
    return out


class _StyleLossFn(torch.autograd.Function):
    """forward: st = lerp(s0, s1, t) -> style forward -> loss and its gradient wrt (u, v) (all HIP kernels).
    backward: the style backward, scaled by the incoming gradient.  With `graph` (a `_StepGraph`), forward replays the captured
    forward + loss + backward and backward has nothing left to do."""

    @staticmethod
    def forward(ctx, model: StyleModel, osl_w, del_w, graph, s1, labels, t, s0, *params):
        B = s1.shape[0]
        L = _loss_ws(model, B, s1.device)
        for k, src in (("s1", s1), ("labels", labels), ("t", t), ("s0", s0)):          # plan-owned static inputs
            L[k].copy_(src.detach().reshape(L[k].shape))
        if graph is not None:
            graph.run(model, L, osl_w, del_w)
        else:
            _step_body(model, L, osl_w, del_w, backward=False)
        out = L["out"].clone()
        ctx.model, ctx.loss_ws, ctx.nparams, ctx.done = model, L, len(params), graph is not None
        return out[0], out[1], out[2], out[3]

    @staticmethod
    def backward(ctx, g_loss, *_):
        if not ctx.done:
            model, L = ctx.model, ctx.loss_ws
            model.attach_grads()
            if g_loss is not None:          # autograd glue: scale the seed gradient (1.0 for loss.backward())
                L["du"].mul_(g_loss)
                L["dv"].mul_(g_loss)
            model.train_backward(L["du"], L["dv"].view(L["dv"].shape[0], -1))
        return (None,) * 8 + (None,) * ctx.nparams


def _loss_ws(model: StyleModel, B: int, dev) -> Dict[str, torch.Tensor]:
    ws = model._train_ws(B, model._dtype(), dev)
    L = ws.get("loss")
    if L is None:
        S = model.style_dim
        z = lambda *shape: torch.zeros(*shape, dtype=torch.float32, device=dev)
        L = ws["loss"] = {"s1": z(B, S, 1), "s0": z(B, S, 1), "t": z(B), "labels": z(B, 5), "st": z(B, S, 1), "dsq": z(B), "sums": z(B, 3),
                          "u": z(B), "v": z(B, S, 1), "dv": z(B, S, 1), "du": z(B), "out": z(4)}
        model._det_flush(L["dsq"], L["sums"], register=True)
    return L


def _step_body(model: StyleModel, L, osl_w: float, del_w: float, backward: bool):
    """The launch sequence of one step on the plan-owned buffers `L`: nothing here allocates, so it can be captured."""
    B, S = L["s1"].shape[0], L["s1"].shape[1]
    L["dsq"].zero_()
    L["sums"].zero_()
    ops.make_xt(L["s0"], L["s1"], L["t"], L["st"], L["dsq"])
    model.train_forward(L["st"].view(B, S), L["labels"], L["u"], L["v"].view(B, S))
    model._det_flush(L["dsq"])                             # (OD_DETERMINISTIC: make_xt's per-sample sums, read by loss_grad)
    ops.loss_grad(L["st"], L["s1"], L["u"], L["v"], L["dsq"], L["dv"], L["sums"], model.c0, osl_w, del_w)
    model._det_flush(L["sums"])
    ops.loss_finalize(L["sums"], L["dsq"], L["u"], L["out"], L["du"], model.c0, osl_w, del_w)
    if backward:
        model.train_backward(L["du"], L["dv"].view(B, S))


class _StepGraph:
    """forward + loss + backward of one training step as one hipGraph (graph.CapturedLoop): one linear stream, inputs in plan-owned
    static buffers, keyed by (B, dtype, the arena's and its gradient buffer's addresses, the deterministic mode).  A call with the same
    key replays; another key captures anew.  The optimizer pass stays a normal launch (its learning rate is a host scalar)."""

    def __init__(self):
        self.key, self.loop, self.captures = None, None, 0

    def run(self, model: StyleModel, L, osl_w, del_w):
        from . import det
        from .graph import CapturedLoop
        g = model.attach_grads()
        dev = g.device
        key = (L["s1"].shape[0], model._dtype(), model.arena.data.data_ptr(), g.data_ptr(), L["out"].data_ptr(), det.enabled(), osl_w, del_w)
        if key != self.key:
            self.close()
            # a first, un-captured run loads every kernel and makes every lazy allocation and registration; the gradients it
            # accumulated are taken back
            saved = g.clone()
            _step_body(model, L, osl_w, del_w, backward=True)
            g.copy_(saved)
            self.loop = CapturedLoop(lambda: _step_body(model, L, osl_w, del_w, backward=True), dev)
            self.key = key
            self.captures += 1
        self.loop.begin()
        self.loop.replay()
        self.loop.end()

    def close(self):
        if self.loop is not None:
            self.loop.close()
        self.key, self.loop = None, None
