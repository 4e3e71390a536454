"""`fit-denoiser` / `fit-style` / `fit-latent` — the training shell around `DiffusionTrainer`, `StyleTrainer` and `LatentTrainer`.

The reference drives its LightningModule with `LightningCLI` + `pytorch_lightning.Trainer`
(osu_dreamer/scripts/fit_denoiser.py:17-32) configured by models/diffusion/model.yml:3-40.
Lightning is not installed on the MI355X image, so this module implements exactly the subset
that config uses, calling the same hooks in the same order:

  seed_everything · precision bf16-mixed (autocast) · gradient_clip_val (global norm, fused into
  the optimizer pass) · AdamW + LambdaLR stepped per batch · on_train_batch_end (EMA) ·
  validation over full maps with the EMA weights · ModelCheckpoint(monitor=val/loss, mode=min,
  save_top_k=1) · resume from --ckpt-path · log_every_n_steps · devices N (one process per GPU,
  gradient exchange by osu_dreamer_amd.ddp.GradBucketReducer over RCCL) · accumulate_grad_batches
  (the denoiser only; Trainer.train_group).

Checkpoints keep Lightning's layout (`state_dict`, `hyper_parameters`, `optimizer_states`,
`lr_schedulers`, `global_step`, `epoch`) so `export-inference` (models/inference/artifact.py)
reads them unchanged.

`fit-style` (osu_dreamer/scripts/fit_style.py, models/style/model.yml) drives `StyleTrainer` through the same shell: the checkpoint
monitor is `val/energy_dist` (mode min), and validation goes through the module's epoch hooks (on_validation_epoch_start /
validation_step / on_validation_epoch_end), which log every value themselves.  It trains on one device, as the reference does.

`fit-latent` (osu_dreamer/scripts/fit_latent.py, models/latent/model.yml) drives `LatentTrainer` the same way over `BeatmapDataModule`:
ModelCheckpoint and EarlyStopping on `eval/score` with mode max (`monitor_mode`, `early_stop_patience`, `early_stop_min_delta`), one device.
"""
from __future__ import annotations

import argparse
import contextlib
import dataclasses
import json
import os
import random
import time
from typing import Any, Dict, Optional

import numpy as np
import torch
import yaml

from . import _lib, launch
from .data import LatentDataModule
from .lr_schedule import LRScheduleArgs
from .model import BackboneArgs, DiffusionModelArgs
from .train import DiffusionTrainer

DEFAULT_CONFIG = os.path.join(os.path.dirname(os.path.abspath(__file__)), "model.yml")
DEFAULT_STYLE_CONFIG = os.path.join(os.path.dirname(os.path.abspath(__file__)), "style.yml")
DEFAULT_LATENT_CONFIG = os.path.join(os.path.dirname(os.path.abspath(__file__)), "latent.yml")


def seed_everything(seed) -> int:
    seed = 0 if seed is True else int(seed)
    random.seed(seed)
    np.random.seed(seed)
    torch.manual_seed(seed)
    return seed


def _plain(o):
    if dataclasses.is_dataclass(o):
        return {k: _plain(v) for k, v in dataclasses.asdict(o).items()}
    if isinstance(o, dict):
        return {k: _plain(v) for k, v in o.items()}
    return o


class Trainer:
    def __init__(self, max_epochs: int = -1, max_steps: int = -1, precision: str = "bf16-mixed",
                 gradient_clip_val: Optional[float] = None, log_every_n_steps: int = 5,
                 val_check_interval: Optional[int] = None, limit_val_batches: Optional[int] = None,
                 default_root_dir: str = "runs/denoiser", accelerator: str = "gpu", devices: int = 1,
                 enable_checkpointing: bool = True, monitor: str = "val/loss", monitor_mode: str = "min",
                 early_stop_patience: Optional[int] = None, early_stop_min_delta: Optional[float] = None,
                 accumulate_grad_batches: int = 1, **_ignored):
        self.max_epochs, self.max_steps = max_epochs, max_steps
        if int(accumulate_grad_batches) != accumulate_grad_batches or accumulate_grad_batches < 1:
            raise ValueError(f"trainer.accumulate_grad_batches must be an integer >= 1, got {accumulate_grad_batches!r}")
        self.accumulate_grad_batches = int(accumulate_grad_batches)   # micro-batches per optimizer step (train_group)
        self.precision = str(precision)
        self.gradient_clip_val = gradient_clip_val
        self.log_every_n_steps = log_every_n_steps
        self.val_check_interval = val_check_interval
        self.limit_val_batches = limit_val_batches
        self.root = default_root_dir
        self.enable_checkpointing = enable_checkpointing
        self.monitor = monitor                        # ModelCheckpoint(monitor=..., mode=monitor_mode, save_top_k=1)
        if monitor_mode not in ("min", "max"):
            raise ValueError(f"monitor_mode must be 'min' or 'max', got {monitor_mode!r}")
        self.monitor_mode = monitor_mode
        self._worst = float("inf") if monitor_mode == "min" else float("-inf")
        self.global_step, self.epoch = 0, 0
        self.best_val = self._worst
        # EarlyStopping(monitor=..., mode=monitor_mode, patience, min_delta): stop after `patience` validations in a row that did not
        # improve on the best one by more than min_delta
        self.early_stop_patience = early_stop_patience
        self.early_stop_min_delta = float(early_stop_min_delta or 0.0)
        self._stop_best, self._stop_wait, self.should_stop = self._worst, 0, False
        # `devices: N` = N ranks, one per GPU (model.yml:11).  The ranks are started by the CLI (`python -m osu_dreamer_amd
        # fit-denoiser` -> launch.spawn_ranks_if_needed) or by the caller's own torchrun, before anything touches the GPU; inside a rank
        # WORLD_SIZE and `devices` must agree in BOTH directions (devices: 1 under a 4-rank torchrun is a mistake, not a 4-GPU run).
        self.devices = launch.parse_devices(devices)
        self.world = int(os.environ.get("WORLD_SIZE", "1"))
        if self.world != self.devices:
            raise RuntimeError(f"trainer.devices={self.devices} but WORLD_SIZE={self.world}: start the run with "
                               "`python -m osu_dreamer_amd fit-denoiser` (it spawns one rank per device) or under "
                               f"`torchrun --nproc-per-node {self.devices}`, and keep trainer.devices equal to the rank count")
        if early_stop_patience is not None and self.world > 1:
            raise RuntimeError("early stopping is decided on rank 0's validation: it is implemented for one device")
        self.rank = int(os.environ.get("RANK", "0"))
        self.local_rank = int(os.environ.get("LOCAL_RANK", "0"))
        self.history = []

    # ------------------------------------------------------------------
    def _autocast(self, device):
        # "16-mixed" (Lightning: fp16 autocast + GradScaler): here bf16 compute with the attention core on IEEE-half operands
        # (module.diffusion.attn_dtype = float16, set in _fit): accumulation is fp32 everywhere and dO is re-scaled by a power of two
        # inside od_flash_attn_bwd_fused, so no loss scaling is needed
        if self.precision.startswith("bf16") or self.precision.startswith("16"):
            return torch.autocast(device.type, dtype=torch.bfloat16)
        return torch.autocast(device.type, enabled=False)

    def _to(self, batch, device):
        if hasattr(batch, "lengths"):      # a ragged batch: the lengths (and a group's row offsets) stay on the host, the engine plans its
            host = ("lengths", "offs")     # varlen calls with them
            return type(batch)(*(t if k in host else t.to(device, non_blocking=True) for k, t in zip(batch._fields, batch)))
        return tuple(t.to(device, non_blocking=True) for t in batch)

    def save_checkpoint(self, path, module, opt, sched):
        ckpt = {
            "state_dict": module.state_dict(),
            "hyper_parameters": _plain(module.hparams_dict),
            "optimizer_states": [opt.state_dict()],
            "lr_schedulers": [sched.state_dict()],
            "global_step": self.global_step, "epoch": self.epoch, "best_val": self.best_val,
        }
        os.makedirs(os.path.dirname(path), exist_ok=True)
        tmp = path + ".tmp"
        torch.save(ckpt, tmp)
        os.replace(tmp, path)

    def validate(self, module, datamodule, device):
        sums: Dict[str, float] = {}
        n = 0
        was_training = module.training
        module.eval()                                 # Lightning runs validation in eval mode (Dropout1d off)
        # by_epoch: the module gathers its batches and logs at the end of the validation epoch (StyleTrainer, style/train.py:111-150), so
        # autocast covers that end and not the steps; otherwise every step runs under autocast and returns logs to average
        by_epoch = getattr(module, "validates_by_epoch", False)
        if by_epoch:
            module.on_validation_epoch_start()
        loader = datamodule.val_dataloader()
        # a feed that groups maps (resident.ResidentLatentValFeed) plans over the first limit_val_batches MAPS itself: the limit keeps
        # meaning maps, as with the batch-1 loaders, where it counts batches
        by_maps = hasattr(loader, "limit")
        if by_maps:
            loader.limit(self.limit_val_batches)
        for i, batch in enumerate(loader):
            if not by_maps and self.limit_val_batches is not None and i >= self.limit_val_batches:
                break
            with contextlib.nullcontext() if by_epoch else self._autocast(device):
                logs = module.validation_step(self._to(batch, device), i)
            if by_epoch:
                continue
            vals = list(logs.values())
            if vals and vals[0].dim() == 1:           # a group's per-map values, name -> (G,): ONE read, then the maps in their order
                table = torch.stack(vals).cpu().tolist()
                for j in range(len(table[0])):
                    for k, row in zip(logs, table):
                        sums[k] = sums.get(k, 0.0) + row[j]
                n += len(table[0])
            else:
                for k, v in logs.items():
                    sums[k] = sums.get(k, 0.0) + float(v)
                n += 1
        if by_epoch:
            with self._autocast(device):
                out = {k: float(v) for k, v in module.on_validation_epoch_end().items()}
        else:
            out = {f"val/{k}": v / max(n, 1) for k, v in sums.items()}
        module.train(was_training)
        return out

    def fit(self, module: DiffusionTrainer, datamodule, ckpt_path: Optional[str] = None):
        device = _lib.training_device(self.local_rank, "training")
        if device.type == "cuda":
            torch.cuda.set_device(device)
        own_group = False
        if self.world > 1:
            import torch.distributed as dist
            if not dist.is_initialized():
                dist.init_process_group("nccl" if device.type == "cuda" else "gloo",
                                        **({"device_id": device} if device.type == "cuda" else {}))
                own_group = True
        try:
            out = self._fit(module, datamodule, ckpt_path, device)
        except BaseException:
            # failure (possibly a dead peer): nothing that waits for the device or for other ranks — abort the RCCL communicator and let
            # the exception end the process; the launcher (torchrun agent) then stops the remaining ranks and returns non-zero
            self._close_reducer(module, abort=True)
            raise
        # orderly teardown: drain the device, destroy the communicator the C ABI created, then the process group — but only a group this
        # call initialised (left to interpreter exit the order is arbitrary and RCCL can hang or abort there)
        if device.type == "cuda":
            torch.cuda.synchronize()
        self._close_reducer(module, abort=False)
        if own_group:
            import torch.distributed as dist
            dist.destroy_process_group()
        return out

    @staticmethod
    def _close_reducer(module, abort: bool):
        net = getattr(module, "diffusion", None)
        reducer = getattr(net, "_reducer", None)
        if reducer is not None:
            try:
                reducer.close(abort=abort)
            except Exception:
                if not abort:         # an abort is already on the way out with the failure that caused it
                    raise
            net._reducer = None

    def train_group(self, module, opt, sched, batches, device, batch_idx: int = 0):
        """One optimizer step on `batches` (already on `device`): the group of micro-batches of gradient accumulation, or the one batch of a
        plain step.  With song counts B_1 .. B_m, micro-batch i's loss is scaled by B_i / sum(B) before backward() — a scale _TrainLossFn
        applies to du / dv on the device — so the gradient left in the arena is the mean over all sum(B) songs: what one step on the union
        batch computes (for a ragged group exactly the union's ragged step; for equal counts Lightning's 1 / m).  zero_grad, the clip, the
        optimizer / scheduler step, the EMA and global_step happen once; a data-parallel reducer exchanges each bucket once, during the last
        backward.  The logged train/* values are the same weighted means.  One batch: no scale, the launch sequence of a plain step.
        Returns the step's train/* logs (device scalars)."""
        m = len(batches)
        if m < 1:
            raise ValueError("train_group needs at least one batch")
        if m > 1 and not hasattr(module, "diffusion"):
            raise RuntimeError("accumulate_grad_batches > 1 is implemented for the denoiser only: the style and latent models hand out their "
                               "gradients as views of one step's buffer, which the next micro-batch would overwrite")
        songs = [int(b[1].size(0)) for b in batches] if m > 1 else [1]
        reducer = getattr(getattr(module, "diffusion", None), "_reducer", None)
        means: Dict[str, Any] = {}
        opt.zero_grad()
        for i, batch in enumerate(batches):
            quiet = reducer.no_sync() if reducer is not None and i + 1 < m else contextlib.nullcontext()
            with quiet:
                with self._autocast(device):
                    loss = module.training_step(batch, batch_idx + i)
                if m > 1:
                    w = songs[i] / sum(songs)
                    loss = loss * w
                    for k, v in module._logged.items():
                        if k.startswith("train/"):
                            means[k] = v * w + means.get(k, 0.0)
                loss.backward()
        if m > 1:
            module._logged.update(means)
        opt.step()
        sched.step()
        module.on_train_batch_end()
        self.global_step += 1
        return {k: v for k, v in getattr(module, "_logged", {}).items() if k.startswith("train/")}

    def _fit(self, module, datamodule, ckpt_path, device):
        reducer = None
        if self.accumulate_grad_batches > 1 and not hasattr(module, "diffusion"):
            raise RuntimeError(f"trainer.accumulate_grad_batches={self.accumulate_grad_batches} is implemented for fit-denoiser only")
        module.gradient_clip_val = self.gradient_clip_val
        module.to(device)
        if self.precision.startswith("16") and hasattr(module, "diffusion"):
            for m in (module.diffusion, module.diffusion_ema.module):
                m.attn_dtype = torch.float16
        cfg = module.configure_optimizers()
        opt, sched = cfg["optimizer"], cfg["lr_scheduler"]["scheduler"]
        if ckpt_path:
            ck = torch.load(ckpt_path, map_location=device, weights_only=False)
            module.load_state_dict(ck["state_dict"])
            opt.load_state_dict(ck["optimizer_states"][0])
            sched.load_state_dict(ck["lr_schedulers"][0])
            self.global_step, self.epoch = ck["global_step"], ck["epoch"]
            self.best_val = ck.get("best_val", self._worst)
        from .ddp import StepAgreement
        if self.world > 1:
            if not hasattr(module, "diffusion"):
                raise RuntimeError("data-parallel training is implemented for the denoiser only (GradBucketReducer follows its arena's segments)")
            from .ddp import GradBucketReducer
            reducer = GradBucketReducer(module.diffusion)
            reducer.broadcast_state(opt, module.diffusion_ema, src=0)     # weights, AdamW moments, EMA: rank 0's
        agree = StepAgreement(self.world)
        log_path = os.path.join(self.root, "metrics.jsonl")
        if self.rank == 0:
            os.makedirs(self.root, exist_ok=True)
        t_last = time.time()
        done = False
        while not done:
            it = iter(datamodule.train_dataloader())
            batch_idx, dry = 0, False
            while not dry:
                # the optimizer step's micro-batches: up to accumulate_grad_batches of them, drawn before any of them runs (their song
                # counts weight them).  Uneven shards: the ranks agree before every draw, so the group — and with it the epoch — ends for
                # every rank as soon as one rank has no batch left; the epoch's last, shorter group still makes a step, an empty one none
                group = []
                while len(group) < self.accumulate_grad_batches:
                    batch = next(it, None)
                    if not agree.all_have(batch is not None):
                        dry = True
                        break
                    group.append(self._to(batch, device))
                if not group:
                    break
                self.train_group(module, opt, sched, group, device, batch_idx)
                batch_idx += len(group)
                if self.global_step % self.log_every_n_steps == 0:
                    opt.check_device_status()          # EVERY rank: a failed launch on one rank must end the job, not train on
                if self.global_step % self.log_every_n_steps == 0 and self.rank == 0:
                    rec = {"step": self.global_step, "epoch": self.epoch, "lr": opt.param_groups[0]["lr"],
                           "s_per_step": (time.time() - t_last) / self.log_every_n_steps,
                           **{k: float(v) for k, v in module._logged.items() if k.startswith("train/")}}
                    t_last = time.time()
                    self.history.append(rec)
                    with open(log_path, "a") as f:
                        f.write(json.dumps(rec) + "\n")
                if self.val_check_interval and self.global_step % self.val_check_interval == 0:
                    self._validate_and_checkpoint(module, datamodule, device, opt, sched)
                if self.should_stop or 0 < self.max_steps <= self.global_step:
                    done = True
                    break
            self.epoch += 1
            if not self.val_check_interval:
                self._validate_and_checkpoint(module, datamodule, device, opt, sched)
            if self.should_stop or 0 < self.max_epochs <= self.epoch:
                done = True
        return self.history

    def _validate_and_checkpoint(self, module, datamodule, device, opt, sched):
        opt.check_device_status()                      # never checkpoint past a failed launch
        val = self.validate(module, datamodule, device)
        if self.rank != 0:
            return
        self.history.append({"step": self.global_step, **val})
        with open(os.path.join(self.root, "metrics.jsonl"), "a") as f:
            f.write(json.dumps({"step": self.global_step, **val}) + "\n")
        score = val.get(self.monitor, self._worst)
        if self.enable_checkpointing and self._better(score, self.best_val):
            self.best_val = val[self.monitor]
            self.save_checkpoint(os.path.join(self.root, "checkpoints", "best.ckpt"), module, opt, sched)
        if self.early_stop_patience is not None:
            if self._better(score, self._stop_best, self.early_stop_min_delta):
                self._stop_best, self._stop_wait = score, 0
            else:
                self._stop_wait += 1
                self.should_stop = self._stop_wait >= self.early_stop_patience

    def _better(self, score: float, best: float, min_delta: float = 0.0) -> bool:
        return score + min_delta < best if self.monitor_mode == "min" else score - min_delta > best


def trainer_kwargs(cfg: Dict[str, Any], command: str, **defaults) -> Dict[str, Any]:
    """The `trainer:` block as Trainer's keywords: without the keys only Lightning reads, with the command's `defaults`.  fit-style and
    fit-latent train on one device and cannot accumulate: either key set otherwise is an error, not a key that is dropped."""
    t = dict(cfg.get("trainer", {}))
    for k in ("callbacks", "logger", "enable_progress_bar", "enable_model_summary", "benchmark"):
        t.pop(k, None)
    if t.get("accumulate_grad_batches") is None:
        t.pop("accumulate_grad_batches", None)
    if command == "fit-denoiser":
        return t
    k = t.pop("accumulate_grad_batches", 1)
    if k != 1:
        raise RuntimeError(f"trainer.accumulate_grad_batches={k} is not implemented for {command}: the model's backward hands out views of a "
                           "per-step gradient buffer, so a second micro-batch would overwrite the first one's gradients instead of adding to "
                           "them.  Set trainer.accumulate_grad_batches: 1 (or drop the key); fit-denoiser accumulates")
    for key, v in defaults.items():
        t.setdefault(key, v)
    if launch.parse_devices(t.get("devices", 1)) > 1:
        raise RuntimeError(f"{command} trains on one device (trainer.devices={t['devices']}): the reference trains the {command[4:]} model on "
                           "one GPU, and the gradient exchange (GradBucketReducer) is tied to the denoiser's arena")
    return t


def build_from_config(cfg: Dict[str, Any]):
    m = dict(cfg["model"])
    da = dict(m["diffusion_args"])
    da["backbone_args"] = BackboneArgs(**da["backbone_args"])
    m["diffusion_args"] = DiffusionModelArgs(**da)
    m["schedule_args"] = LRScheduleArgs(**m["schedule_args"])
    return DiffusionTrainer(**m), Trainer(**trainer_kwargs(cfg, "fit-denoiser"))


def refuse_ragged_data_parallel(cfg: Dict[str, Any], devices: int):
    """Ragged training (data.seq_len: null) is implemented and tested for one device."""
    data = cfg.get("data") or {}
    if devices > 1 and "seq_len" in data and data["seq_len"] is None:
        raise RuntimeError(f"ragged training (data.seq_len: null) runs on one device, got trainer.devices={devices}: data-parallel ragged "
                           "steps are not implemented.  Train whole maps with trainer.devices: 1, or fixed windows (an integer "
                           "data.seq_len) on several devices")


def pop_resident(data: Dict[str, Any], trainer: "Trainer") -> Optional[Dict[str, Any]]:
    """Takes `resident` and `resident_max_gb` out of the `data:` block.  None: the host loader; else the resident data module's `device`
    and `resident_max_gb` keywords."""
    resident, max_gb = data.pop("resident", False), data.pop("resident_max_gb", None)
    if not resident:
        if max_gb is not None:
            raise ValueError("data.resident_max_gb bounds the resident store: set data.resident: true, or drop the key")
        return None
    if data.get("num_workers") and trainer.rank == 0:
        print(f"data.resident: batches are gathered on the device, data.num_workers={data['num_workers']} is ignored for training")
    return dict(device=_lib.training_device(trainer.local_rank, "data.resident"), resident_max_gb=max_gb)


def pop_resident_val(data: Dict[str, Any], resident: Optional[Dict[str, Any]]) -> Dict[str, Any]:
    """Takes `resident_val` and `val_frame_budget` out of the `data:` block, as the resident data modules' keywords.  Both validate from a
    second resident store: without `resident` (pop_resident's answer None) either key is refused, and so is a budget without `resident_val`."""
    resident_val, val_budget = data.pop("resident_val", False), data.pop("val_frame_budget", None)
    if resident is None:
        if resident_val or val_budget is not None:
            raise ValueError("data.resident_val / data.val_frame_budget validate from the resident store: set data.resident: true, or drop "
                             "the keys")
        return {}
    if val_budget is not None and not resident_val:
        raise ValueError("data.val_frame_budget sizes the groups of the resident validation: set data.resident_val: true, or drop the key")
    return dict(resident_val=bool(resident_val), val_frame_budget=val_budget)


def build_latent_data(data: Dict[str, Any], trainer: "Trainer", style_only: bool = False, val_batches: Optional[int] = None, **shard):
    """The `data:` block -> its data module.  `data.resident: true` keeps the training set on the device (resident.py: every file read once,
    batches gathered by od_feed_gather), within `data.resident_max_gb` when that is set; fit-style's store holds the style fields only.
    `data.resident_val: true` (with data.resident, fit-denoiser) keeps the held-out maps there too and validates them in groups of at most
    `data.val_frame_budget` padded frames (default 131 072), each map cut into the model's `val_batches` segments and padded to
    `data.pad_multiple`."""
    resident = pop_resident(data, trainer)
    val = pop_resident_val(data, resident)
    if resident is None:
        return LatentDataModule(**data, **shard)
    from .resident import STYLE_FIELDS, ALL_FIELDS, ResidentLatentDataModule
    return ResidentLatentDataModule(**data, **shard, **resident, **val, val_batches=val_batches,
                                    fields=STYLE_FIELDS if style_only else ALL_FIELDS)


def load_config(config: str, overrides: Dict[str, Any]) -> Dict[str, Any]:
    """The YAML with the `section__key=value` overrides applied (e.g. data__data_path="..."), and everything seeded as it asks."""
    with open(config) as f:
        cfg = yaml.safe_load(f)
    for k, v in overrides.items():
        sec, key = k.split("__")
        cfg.setdefault(sec, {})[key] = v
    if cfg.get("seed_everything") not in (None, False):
        seed_everything(cfg["seed_everything"])
    return cfg


def fit_denoiser(config: str = DEFAULT_CONFIG, ckpt_path: Optional[str] = None, **overrides):
    """begin a training run for the diffusion model (reference: scripts/fit_denoiser.py:17-32)."""
    cfg = load_config(config, overrides)
    devices = launch.parse_devices(cfg.get("trainer", {}).get("devices", 1))
    refuse_ragged_data_parallel(cfg, devices)
    if devices > 1 and launch.world_from_env() is None:
        # this function runs INSIDE a rank; only the CLI (main(), below) starts ranks, because that has to happen in a process
        # that never touches the GPU
        raise RuntimeError(f"fit_denoiser() with trainer.devices={devices} must run inside a rank: use `python -m osu_dreamer_amd "
                           f"fit-denoiser` (it starts the {devices} ranks) or `torchrun --nproc-per-node {devices}`")
    module, trainer = build_from_config(cfg)
    data = build_latent_data(dict(cfg["data"]), trainer, val_batches=module.val_batches, rank=trainer.rank, world_size=trainer.world)
    trainer.fit(module, data, ckpt_path=ckpt_path)
    return module, trainer


def build_style_from_config(cfg: Dict[str, Any]):
    from .style_train import StyleTrainer
    m = dict(cfg["model"])
    m["schedule_args"] = LRScheduleArgs(**(m.get("schedule_args") or {}))       # models/style/model.yml leaves the schedule at its defaults
    return StyleTrainer(**m), Trainer(**trainer_kwargs(cfg, "fit-style", monitor="val/energy_dist", default_root_dir="runs/style"))


def fit_style(config: str = DEFAULT_STYLE_CONFIG, ckpt_path: Optional[str] = None, **overrides):
    """begin a training run for the style model (reference: scripts/fit_style.py:17-32)."""
    cfg = load_config(config, overrides)
    module, trainer = build_style_from_config(cfg)
    data = build_latent_data(dict(cfg["data"]), trainer, style_only=True)
    trainer.fit(module, data, ckpt_path=ckpt_path)
    return module, trainer


def build_latent_from_config(cfg: Dict[str, Any]):
    from .latent_train import LatentTrainer
    m = dict(cfg["model"])
    m["schedule_args"] = LRScheduleArgs(**(m.get("schedule_args") or {}))
    t = trainer_kwargs(cfg, "fit-latent", monitor="eval/score", monitor_mode="max", default_root_dir="runs/latent")
    module, trainer = LatentTrainer(**m), Trainer(**t)
    if trainer.precision.startswith("bf16"):
        module.latent.compute_dtype = torch.bfloat16        # LatentModel does not follow autocast: its compute type is set here
    return module, trainer


def build_beatmap_data(data: Dict[str, Any], trainer: "Trainer", val_pad_multiple: Optional[int] = None):
    """fit-latent's `data:` block -> its data module.  `data.resident: true` keeps the training set on the device as the integers of its
    files (resident.py: every spec.npy and map read once, batches dequantised, flipped and padded by od_feed_gather_quant), within
    `data.resident_max_gb` when that is set.  `data.resident_val: true` (with data.resident) keeps the held-out maps there too and
    validates them in ragged groups of at most `data.val_frame_budget` padded frames, each map padded to `val_pad_multiple` (the
    trainer's 2 x chunk_size)."""
    from .data import BeatmapDataModule
    resident = pop_resident(data, trainer)
    val = pop_resident_val(data, resident)
    if resident is None:
        return BeatmapDataModule(**data)
    from .resident import ResidentBeatmapDataModule
    return ResidentBeatmapDataModule(**data, **resident, **val, val_pad_multiple=val_pad_multiple)


def fit_latent(config: str = DEFAULT_LATENT_CONFIG, ckpt_path: Optional[str] = None, **overrides):
    """begin a training run for the latent model (reference: scripts/fit_latent.py, models/latent/model.yml)."""
    cfg = load_config(config, overrides)
    module, trainer = build_latent_from_config(cfg)
    data = build_beatmap_data(dict(cfg["data"]), trainer, val_pad_multiple=2 * module.latent.chunk_size)
    trainer.fit(module, data, ckpt_path=ckpt_path)
    return module, trainer


def main(argv=None):
    ap = argparse.ArgumentParser(prog="osu_dreamer_amd")
    sub = ap.add_subparsers(dest="cmd", required=True)
    fits = {"fit-denoiser": ("diffusion", DEFAULT_CONFIG, fit_denoiser), "fit-style": ("style", DEFAULT_STYLE_CONFIG, fit_style),
            "fit-latent": ("latent", DEFAULT_LATENT_CONFIG, fit_latent)}
    for cmd, (model, config, _) in fits.items():
        f = sub.add_parser(cmd, help=f"begin a training run for the {model} model")
        f.add_argument("-c", "--config", default=config)
        f.add_argument("--ckpt-path", default=None)
    from . import encode_latents as encode_cmd
    from . import predict as predict_cmd
    encode_cmd.add_parser(sub)
    predict_cmd.add_parser(sub)
    a = ap.parse_args(argv)
    if a.cmd == "predict":
        return predict_cmd.run(a)
    if a.cmd == "encode-latents":
        return encode_cmd.run(a)
    if a.cmd == "fit-denoiser":
        with open(a.config) as fh:
            cfg = yaml.safe_load(fh)
        devices = launch.parse_devices((cfg.get("trainer") or {}).get("devices", 1))
        refuse_ragged_data_parallel(cfg, devices)       # before any rank is started
        # trainer.devices N > 1: this process only starts the N ranks (children; nothing here has touched the GPU)
        rc = launch.spawn_ranks_if_needed(devices, ["fit-denoiser", "-c", a.config] + (["--ckpt-path", a.ckpt_path] if a.ckpt_path else []),
                                          module="osu_dreamer_amd")
        if rc is not None:
            raise SystemExit(rc)
    fits[a.cmd][2](a.config, a.ckpt_path)


if __name__ == "__main__":
    main()
