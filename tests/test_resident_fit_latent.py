"""`fit-latent` with `data.resident: true`: the tiny configuration of tests/test_fit_latent.py trained from the resident beatmap feed —
finite losses, a validation on the host loader and a checkpoint `encode-latents` loads — and the refusals around the key.  Emulator and
MI355X (the `dev` fixture)."""
import json

import numpy as np
import pytest
import torch
import yaml

from osu_dreamer_amd.data import BeatmapDataModule, write_synthetic_beatmaps
from osu_dreamer_amd.encode_latents import load_latent_ckpt
from osu_dreamer_amd.fit import DEFAULT_LATENT_CONFIG, build_beatmap_data, build_latent_from_config, fit_latent
from osu_dreamer_amd.resident import ResidentBeatmapDataModule
from tools.gen_latent_train_golden import CASES, model_args
from kernel_backend import dev  # noqa: F401

C = CASES["s4r1"]
SEQ, BATCH, STEPS = 4 * C.L, 3, 4


def _cfg(tmp_path, data_dir, **data):
    cfg = yaml.safe_load(open(DEFAULT_LATENT_CONFIG))
    a = model_args(C)
    cfg["model"].update(emb_dim=a["emb_dim"], style_dim=a["style_dim"], n_downs=a["n_downs"], stride=a["stride"], latent_args=a["args"],
                        schedule_args=dict(warmup_init=0.1, warmup_steps=4))
    cfg["data"].update(data_path=str(data_dir), batch_size=BATCH, seq_len=SEQ, num_workers=0, max_val_count=2, **data)
    cfg["trainer"].update(max_steps=STEPS, log_every_n_steps=1, val_check_interval=3, default_root_dir=str(tmp_path / "run"), precision="32")
    return cfg


def test_fit_latent_resident(dev, tmp_path, capsys):
    data_dir = tmp_path / "data"
    write_synthetic_beatmaps(str(data_dir), n_mapsets=12, maps_per_set=1, frames=[150, 131] * 6, seed=3)
    cfg = _cfg(tmp_path, data_dir, resident=True, resident_max_gb=0.01)
    cfg["data"]["num_workers"] = 3
    path = tmp_path / "latent.yml"
    path.write_text(yaml.safe_dump(cfg))
    seen = []
    gather = ResidentBeatmapDataModule.train_dataloader

    def spy(self):
        seen.append(self)
        return gather(self)
    ResidentBeatmapDataModule.train_dataloader = spy
    try:
        module, trainer = fit_latent(str(path))          # 10 training maps: 3 batches per epoch, so step 4 opens epoch 2
    finally:
        ResidentBeatmapDataModule.train_dataloader = gather
    assert "data.num_workers=3 is ignored" in capsys.readouterr().out
    assert len(seen) == 2 and len(seen[0].store) == 10 and seen[0].store.data.device.type == dev.type
    assert trainer.global_step == STEPS
    lines = [json.loads(l) for l in open(tmp_path / "run" / "metrics.jsonl")]
    train = [l for l in lines if "train/loss" in l]
    assert [l["step"] for l in train] == list(range(1, STEPS + 1))
    assert all(np.isfinite(l[k]) for l in train for k in ("train/loss", "train/hit/onset", "train/cursor/pos", "train/cursor/acc", "train/label"))
    val = [l for l in lines if "eval/score" in l]            # the host loader's whole maps
    assert len(val) == 1 and np.isfinite(val[0]["val/loss"]) and np.isfinite(val[0]["eval/score"])
    ckpt = tmp_path / "run" / "checkpoints" / "best.ckpt"
    assert torch.load(ckpt, map_location="cpu", weights_only=False)["global_step"] == 3
    m = load_latent_ckpt(str(ckpt), device=dev)
    batch = next(iter(seen[0].train_dataloader()))
    z, s = m.encode_chart(batch.chart[:, :, :2 * C.L])
    assert bool(torch.isfinite(z).all()) and bool(torch.isfinite(s).all()) and z.shape[0] == BATCH


def test_resident_max_gb_alone_is_refused(tmp_path):
    cfg = _cfg(tmp_path, tmp_path / "data", resident_max_gb=1.0)
    path = tmp_path / "latent.yml"
    path.write_text(yaml.safe_dump(cfg))
    with pytest.raises(ValueError, match="data.resident: true"):
        fit_latent(str(path))


def test_the_key_chooses_the_data_module(dev, tmp_path):
    data_dir = tmp_path / "data"
    write_synthetic_beatmaps(str(data_dir), n_mapsets=4, maps_per_set=1, frames=[150, 131] * 2, seed=3)
    cfg = _cfg(tmp_path, data_dir)
    _, trainer = build_latent_from_config(cfg)
    plain = build_beatmap_data(dict(cfg["data"]), trainer)
    assert type(plain) is BeatmapDataModule and plain.num_workers == 0
    off = build_beatmap_data(dict(cfg["data"], resident=False), trainer)
    assert type(off) is BeatmapDataModule
    on = build_beatmap_data(dict(cfg["data"], resident=True), trainer)
    assert type(on) is ResidentBeatmapDataModule and on.device.type == dev.type and len(on.store) == 3
    with pytest.raises(MemoryError, match="resident_max_gb"):
        build_beatmap_data(dict(cfg["data"], resident=True, resident_max_gb=1e-6), trainer)
