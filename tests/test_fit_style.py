"""`fit-style` plumbing: synthetic latent files on disk -> LatentDataModule -> Trainer.fit(StyleTrainer) -> metrics.jsonl, a checkpoint on
`val/energy_dist` with the reference StyleTrainer's key layout, resume from --ckpt-path, `style_from_checkpoint`."""
import json
import os

import numpy as np
import pytest
import torch
import yaml

from oracle import style_oracle as SO
from osu_dreamer_amd.data import LatentDataModule, write_synthetic_dataset
from osu_dreamer_amd.fit import DEFAULT_STYLE_CONFIG, build_style_from_config, main
from osu_dreamer_amd.inference import style_from_checkpoint
from tools.gen_style_train_golden import style_batch
from kernel_backend import dev  # noqa: F401

GOLDEN = os.path.join(os.path.dirname(__file__), "golden")
D, BATCH = SO.STYLE_TINY, 4


def _cfg(tmp_path, data_dir):
    cfg = yaml.safe_load(open(DEFAULT_STYLE_CONFIG))
    cfg["model"].update(style_dim=D.style_dim, style_args=dict(label_features=D.label_features, h_dim=D.h_dim, depth=D.depth, expand=D.expand))
    cfg["data"].update(data_path=str(data_dir), batch_size=BATCH, num_workers=0, shuffle_buffer_size=1, max_val_count=4)
    cfg["trainer"].update(max_steps=4, log_every_n_steps=1, val_check_interval=3, default_root_dir=str(tmp_path / "run"), precision="32")
    return cfg


def _build(cfg):
    """Module + trainer with un-zeroed weights and the step's draws pinned to the global step."""
    module, trainer = build_style_from_config(cfg)
    module.style.load_state_dict(SO.init_style_params(D, 6))
    module.style_ema.module.load_state_dict(SO.init_style_params(D, 6))
    step = module.training_step

    def pinned(batch, idx):
        b = style_batch(D, BATCH, 1000 + trainer.global_step)
        dev_ = batch[2].device
        return step(batch, idx, t=b["t"].to(dev_), s0=b["s0"].to(dev_), drop=b["drop"].to(dev_))
    module.training_step = pinned
    return module, trainer


def test_shipped_config_carries_the_reference_values():
    cfg = yaml.safe_load(open(DEFAULT_STYLE_CONFIG))
    assert cfg["data"]["batch_size"] == 512 and cfg["data"]["seq_len"] == 1 and cfg["data"]["max_per_map"] == 1
    assert cfg["data"]["shuffle_buffer_size"] == 512
    m = cfg["model"]
    assert m["opt_args"] == dict(lr=3e-4, weight_decay=0.01) and m["label_drop_prob"] == 0.2 and (m["osl_weight"], m["del_weight"]) == (1.0, 30.0)
    assert m["style_dim"] == 32 and m["style_args"] == dict(label_features=128, h_dim=256, depth=8, expand=4)
    assert cfg["trainer"]["precision"] == "bf16-mixed" and cfg["trainer"]["gradient_clip_val"] == 1.0
    assert cfg["trainer"]["monitor"] == "val/energy_dist"


def test_fit_style_synthetic(dev, tmp_path):
    data_dir = tmp_path / "data"
    write_synthetic_dataset(str(data_dir), n_maps=16, frames=8, a_dim=4, emb_dim=2, style_dim=D.style_dim, seed=3)
    cfg = _cfg(tmp_path, data_dir)
    torch.manual_seed(0)
    module, trainer = _build(cfg)
    assert trainer.monitor == "val/energy_dist"
    dm = LatentDataModule(**cfg["data"])
    hist = trainer.fit(module, dm)                          # 12 training maps: 3 batches per epoch, so step 4 opens epoch 2
    train = [h for h in hist if "train/loss" in h]
    assert len(train) == 4 and all(np.isfinite(h["train/loss"]) for h in train)
    assert all(k in train[0] for k in ("train/osl", "train/del", "train/u_mape"))
    val = [h for h in hist if "val/energy_dist" in h]
    assert len(val) == 1 and all(k in val[0] for k in ("val/loss", "val/nn_ratio", "val/cond_recall", "val/sample_spread"))
    assert int(module.style_ema.n_averaged) == 4
    lines = [json.loads(l) for l in open(tmp_path / "run" / "metrics.jsonl")]
    assert any("train/loss" in l for l in lines) and any("val/energy_dist" in l for l in lines)
    path = tmp_path / "run" / "checkpoints" / "best.ckpt"
    ck = torch.load(path, map_location="cpu", weights_only=False)
    assert ck["global_step"] == 3 and ck["best_val"] == pytest.approx(val[0]["val/energy_dist"])
    ref_keys = [str(s) for s in np.load(os.path.join(GOLDEN, "style_train_val_tiny.npz"))["sd_keys"]]
    assert sorted(ck["state_dict"].keys()) == sorted(ref_keys)              # exactly the reference StyleTrainer's key set
    hp = ck["hyper_parameters"]
    assert hp["style_dim"] == D.style_dim and type(hp["style_args"]) is dict
    assert hp["style_args"] == dict(label_features=D.label_features, h_dim=D.h_dim, depth=D.depth, expand=D.expand)
    # the loader gives the checkpoint's EMA model: the same samples as the module that wrote it had at step 3
    m = style_from_checkpoint(str(path), device=dev)
    assert not any(p.requires_grad for p in m.parameters())
    for k, v in m.state_dict().items():
        assert torch.equal(v.cpu(), ck["state_dict"]["style_ema.module." + k]), k
    raw = style_from_checkpoint(str(path), use_ema=False, device=dev)
    assert torch.equal(raw.proj_in.weight.cpu(), ck["state_dict"]["style.proj_in.weight"])
    # resume: step 4 of the resumed run has the loss step 4 of the uninterrupted run had (same data: epoch 2's first batch; same pins)
    module2, trainer2 = _build(cfg)
    trainer2.val_check_interval = None
    trainer2.max_epochs = 1
    trainer2.fit(module2, dm, ckpt_path=str(path))
    assert trainer2.global_step >= 4
    resumed = [h for h in trainer2.history if h.get("step") == 4 and "train/loss" in h]
    assert resumed and resumed[0]["train/loss"] == pytest.approx(train[3]["train/loss"], rel=1e-5)
    assert resumed[0]["lr"] == pytest.approx(train[3]["lr"], rel=1e-12)
    # the EMA module of a trainer and the model loaded from its checkpoint sample alike
    trainer2.save_checkpoint(str(tmp_path / "last.ckpt"), module2, *[c for c in _opt_sched(module2)])
    m2 = style_from_checkpoint(str(tmp_path / "last.ckpt"), device=dev)
    labels = torch.rand(5, 5, generator=torch.Generator().manual_seed(1)).to(dev) * 10
    s_init = torch.randn(5, D.style_dim, generator=torch.Generator().manual_seed(2)).to(dev)
    assert torch.equal(m2.sample(labels, 16, s_init=s_init), module2.style_ema.module.sample(labels, 16, s_init=s_init))


def _opt_sched(module):
    cfg = module.configure_optimizers()
    return cfg["optimizer"], cfg["lr_scheduler"]["scheduler"]


def test_fit_style_refuses_more_than_one_device(tmp_path):
    cfg = _cfg(tmp_path, tmp_path / "data")
    cfg["trainer"]["devices"] = 2
    with pytest.raises(RuntimeError, match="one device"):
        build_style_from_config(cfg)


def test_cli_has_fit_style(tmp_path, capsys):
    with pytest.raises(SystemExit) as e:
        main(["fit-style", "--help"])
    assert e.value.code == 0 and "--ckpt-path" in capsys.readouterr().out
