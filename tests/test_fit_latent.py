"""`fit-latent` plumbing: synthetic beatmaps on disk -> BeatmapDataModule -> Trainer.fit(LatentTrainer) -> metrics.jsonl, a checkpoint on the
largest `eval/score` with the reference LatentTrainer's key layout, which `encode-latents`' loader reads; resume from --ckpt-path; the
trainer shell's `monitor_mode` and early stopping on a stub module with scripted scores."""
import json
import os

import numpy as np
import pytest
import torch
import yaml

from osu_dreamer_amd.data import BeatmapDataModule, write_synthetic_beatmaps
from osu_dreamer_amd.encode_latents import load_latent_ckpt
from osu_dreamer_amd.fit import DEFAULT_LATENT_CONFIG, Trainer, build_latent_from_config, main
from osu_dreamer_amd.optim import ClippedAdamW
from tools.gen_latent_train_golden import CASES, grad_weights, model_args, pins, train_batch
from kernel_backend import dev  # noqa: F401

GOLDEN = os.path.join(os.path.dirname(__file__), "golden")
C = CASES["s4r1"]
SEQ, BATCH = 4 * C.L, 3                  # the golden batches' shape: 3 windows of two 40-frame halves


def _cfg(tmp_path, data_dir):
    cfg = yaml.safe_load(open(DEFAULT_LATENT_CONFIG))
    a = model_args(C)
    cfg["model"].update(emb_dim=a["emb_dim"], style_dim=a["style_dim"], n_downs=a["n_downs"], stride=a["stride"], latent_args=a["args"],
                        schedule_args=dict(warmup_init=0.1, warmup_steps=4))
    cfg["data"].update(data_path=str(data_dir), batch_size=BATCH, seq_len=SEQ, num_workers=0, max_val_count=2)
    cfg["trainer"].update(max_steps=4, log_every_n_steps=1, val_check_interval=3, default_root_dir=str(tmp_path / "run"), precision="32")
    return cfg


def _build(cfg):
    """Module + trainer with the golden weights; every step trains on a seeded batch with seeded draws, keyed by the global step."""
    module, trainer = build_latent_from_config(cfg)
    module.latent.load_state_dict(grad_weights(C))
    step = module.training_step

    def pinned(batch, idx):
        assert batch[0].shape == (BATCH, 72, SEQ) and batch[1].shape == (BATCH, 9, SEQ) and batch[2].shape == (BATCH, 5)
        d = batch[0].device
        b = tuple(t.to(d) for t in train_batch(C, 1000 + trainer.global_step))
        return step(b, idx, **{k: v.to(d) for k, v in pins(C, 2000 + trainer.global_step).items()})
    module.training_step = pinned
    return module, trainer


def test_shipped_config_carries_the_reference_values():
    cfg = yaml.safe_load(open(DEFAULT_LATENT_CONFIG))
    assert cfg["data"] == dict(seq_len=2052, batch_size=32, num_workers=13, max_val_count=64, max_per_map=1)
    m = cfg["model"]
    assert m["opt_args"] == dict(lr=1e-3, weight_decay=0.01) and m["schedule_args"] == dict(warmup_init=0.1, warmup_steps=2000)
    assert (m["s_reg_weight"], m["s_noise"], m["z_noise"], m["z_mask_frac"], m["s_mask_frac"]) == (1e-3, 0.2, 0.2, 0.25, 0.1)
    assert (m["emb_dim"], m["style_dim"], m["n_downs"], m["stride"]) == (6, 32, 3, 3)
    assert m["latent_args"] == dict(h_dim=128, ae_args=dict(n_layers=8, expand=4, radius=2), style_head_dim=64, style_heads=16)
    t = cfg["trainer"]
    assert t["precision"] == "bf16-mixed" and t["gradient_clip_val"] == 1.0 and t["devices"] == 1
    assert (t["monitor"], t["monitor_mode"], t["early_stop_patience"], t["early_stop_min_delta"]) == ("eval/score", "max", 10, 0.001)
    assert t["default_root_dir"] == "runs/latent"
    module, trainer = build_latent_from_config(cfg)
    assert module.latent.compute_dtype == torch.bfloat16 and module.latent.chunk_size == 27 and trainer.best_val == float("-inf")
    assert all(p.requires_grad for p in module.latent.parameters())


def test_fit_latent_synthetic(dev, tmp_path):
    data_dir = tmp_path / "data"
    write_synthetic_beatmaps(str(data_dir), n_mapsets=12, maps_per_set=1, frames=[150, 131] * 6, seed=3)
    cfg = _cfg(tmp_path, data_dir)
    torch.manual_seed(0)
    module, trainer = _build(cfg)
    assert (trainer.monitor, trainer.monitor_mode) == ("eval/score", "max") and module.latent.compute_dtype is None
    dm = BeatmapDataModule(**cfg["data"])
    assert len(dm.val_set.mapsets) == 2 and len(dm.train_set.mapsets) == 10
    hist = trainer.fit(module, dm)                          # 10 training maps: 3 batches per epoch, so step 4 opens epoch 2
    train = [h for h in hist if "train/loss" in h]
    assert len(train) == 4 and all(np.isfinite(h["train/loss"]) for h in train)
    assert all(k in train[0] for k in ("train/hit/onset", "train/cursor/acc", "train/label", "train/s_reg"))
    val = [h for h in hist if "eval/score" in h]
    assert len(val) == 1 and all(k in val[0] for k in ("val/loss", "eval/hit/dice", "eval/cursor/vel/r2", "eval/cursor_px_mae", "eval/z_var_min"))
    lines = [json.loads(l) for l in open(tmp_path / "run" / "metrics.jsonl")]
    assert any("train/loss" in l for l in lines) and any("eval/score" in l for l in lines)
    path = tmp_path / "run" / "checkpoints" / "best.ckpt"
    ck = torch.load(path, map_location="cpu", weights_only=False)
    assert ck["global_step"] == 3 and ck["best_val"] == pytest.approx(val[0]["eval/score"]) and ck["best_val"] > float("-inf")
    ref_keys = [str(s) for s in np.load(os.path.join(GOLDEN, "latent_train_val_tiny.npz"))["sd_keys"]]
    # exactly the reference LatentTrainer's key set: its buffers as recorded, and `latent.` + the keys the reference's LatentModel of these
    # dims takes with strict=True (grad_weights; the recorded list is the `tiny` model's)
    assert sorted(k for k in ck["state_dict"] if not k.startswith("latent.")) == sorted(k for k in ref_keys if not k.startswith("latent."))
    assert sorted(k for k in ck["state_dict"] if k.startswith("latent.")) == sorted("latent." + k for k in grad_weights(C))
    assert ck["state_dict"]["loss_ema_initialized"].dtype == torch.bool and bool(ck["state_dict"]["loss_ema_initialized"])
    hp = ck["hyper_parameters"]
    assert hp["emb_dim"] == C.emb and type(hp["latent_args"]) is dict and hp["latent_args"] == model_args(C)["args"]
    # resume: step 4 of the resumed run has the loss and the LR step 4 of the uninterrupted run had
    module2, trainer2 = _build(cfg)
    trainer2.val_check_interval = None
    trainer2.max_epochs = 1
    trainer2.fit(module2, dm, ckpt_path=str(path))
    assert trainer2.global_step >= 4 and trainer2.best_val >= ck["best_val"]
    resumed = [h for h in trainer2.history if h.get("step") == 4 and "train/loss" in h]
    assert resumed and resumed[0]["train/loss"] == pytest.approx(train[3]["train/loss"], rel=1e-5)
    assert resumed[0]["lr"] == pytest.approx(train[3]["lr"], rel=1e-12)
    # the loader of encode-latents reads the checkpoint as is, and the loaded model encodes as the module's own
    cfg2 = module2.configure_optimizers()
    trainer2.save_checkpoint(str(tmp_path / "last.ckpt"), module2, cfg2["optimizer"], cfg2["lr_scheduler"]["scheduler"])
    m = load_latent_ckpt(str(tmp_path / "last.ckpt"), device=dev)
    chart = train_batch(C, 77)[1][:, :, :2 * C.L].to(dev)
    module2.eval()
    with torch.no_grad():
        z0, s0 = module2.latent.encode_chart(chart)
    z1, s1 = m.encode_chart(chart)
    assert torch.equal(z0, z1) and torch.equal(s0, s1) and not any(p.requires_grad for p in m.parameters())


class _Stub(torch.nn.Module):
    """A module whose validation returns scripted scores."""
    validates_by_epoch = True

    def __init__(self, scores):
        super().__init__()
        self.w = torch.nn.Parameter(torch.ones(1))
        self.scores, self._logged, self.hparams_dict = list(scores), {}, {}

    def configure_optimizers(self):
        opt = ClippedAdamW([self.w], lr=1e-3)
        return {"optimizer": opt, "lr_scheduler": {"scheduler": torch.optim.lr_scheduler.LambdaLR(opt, lambda s: 1.0)}}

    def training_step(self, batch, idx):
        return self.w.pow(2).sum()

    def on_train_batch_end(self):
        pass

    def on_validation_epoch_start(self):
        pass

    def validation_step(self, batch, idx):
        pass

    def on_validation_epoch_end(self):
        return {"score": self.scores.pop(0)}


class _OneBatch:
    def train_dataloader(self):
        return [(torch.zeros(1),)]

    def val_dataloader(self):
        return [(torch.zeros(1),)]


SCORES = [0.1, 0.5, 0.505, 0.3, 0.9, 0.2]


def test_monitor_mode_max_and_early_stopping(dev, tmp_path):
    """max: the checkpoint follows the largest score (0.505 at step 3, no min_delta there); early stopping counts validations that did not
    beat the best by more than min_delta: 0.505 and 0.3 after 0.5 -> stop after the 4th epoch, before 0.9 is ever seen."""
    tr = Trainer(max_epochs=6, monitor="score", monitor_mode="max", early_stop_patience=2, early_stop_min_delta=0.01,
                 default_root_dir=str(tmp_path / "max"), precision="32")
    assert tr.best_val == float("-inf")
    m = _Stub(SCORES)
    tr.fit(m, _OneBatch())
    assert tr.epoch == 4 and tr.should_stop and m.scores == [0.9, 0.2] and tr.best_val == 0.505
    assert torch.load(tmp_path / "max" / "checkpoints" / "best.ckpt", weights_only=False)["global_step"] == 3


def test_monitor_mode_min_is_the_default(dev, tmp_path):
    tr = Trainer(max_epochs=6, monitor="score", default_root_dir=str(tmp_path / "min"), precision="32")
    assert tr.monitor_mode == "min" and tr.best_val == float("inf") and tr.early_stop_patience is None
    m = _Stub(SCORES)
    tr.fit(m, _OneBatch())
    assert tr.epoch == 6 and not tr.should_stop and m.scores == [] and tr.best_val == 0.1
    assert torch.load(tmp_path / "min" / "checkpoints" / "best.ckpt", weights_only=False)["global_step"] == 1
    with pytest.raises(ValueError, match="monitor_mode"):
        Trainer(monitor_mode="largest")


def test_fit_latent_refuses_more_than_one_device(tmp_path):
    cfg = _cfg(tmp_path, tmp_path / "data")
    cfg["trainer"]["devices"] = 2
    with pytest.raises(RuntimeError, match="one device"):
        build_latent_from_config(cfg)


def test_cli_has_fit_latent(tmp_path, capsys):
    with pytest.raises(SystemExit) as e:
        main(["fit-latent", "--help"])
    assert e.value.code == 0 and "--ckpt-path" in capsys.readouterr().out
