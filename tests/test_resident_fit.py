"""`fit-denoiser` and `fit-style` with `data.resident: true`, and one denoiser step on a resident batch against the same step on the
host-collated batch of the same maps.  Tiny models, as tests/test_fit.py and tests/test_fit_style.py; emulator and MI355X (the `dev` fixture)."""
import json

import numpy as np
import pytest
import torch
import yaml

from oracle import denoiser_oracle as O
from oracle import style_oracle as SO
from osu_dreamer_amd import det
from osu_dreamer_amd.data import LatentBatch, collate_ragged, load_latents, write_synthetic_dataset
from osu_dreamer_amd.fit import DEFAULT_STYLE_CONFIG, fit_denoiser, fit_style
from osu_dreamer_amd.resident import ResidentLatentDataModule
from kernel_backend import dev  # noqa: F401
from test_model_parity import make_trainer
from test_ragged_train import _ragged_cfg

STEPS = 4


def test_fit_denoiser_resident_frame_budget(dev, tmp_path, capsys):
    """test_bucketed_batches' command test with the training set resident: four steps over frame-budget batches gathered on the device,
    one metrics record each, every loss finite, one validation (the host loader's) and its checkpoint."""
    cfg = _ragged_cfg(tmp_path, dev)
    cfg["data"].update(batch_size=4, batch_frames=256, bucket_pool=6, resident=True, resident_max_gb=0.5, num_workers=3)
    cfg["trainer"].update(max_steps=STEPS, val_check_interval=STEPS)          # an epoch is three batches: step 4 opens the second
    path = tmp_path / "resident.yml"
    path.write_text(yaml.safe_dump(cfg))
    module, trainer = fit_denoiser(str(path))
    assert "data.num_workers=3 is ignored" in capsys.readouterr().out
    assert trainer.global_step == STEPS and int(module.diffusion_ema.n_averaged) == STEPS
    lines = [json.loads(l) for l in open(tmp_path / "run" / "metrics.jsonl")]
    train = [l for l in lines if "train/loss" in l]
    assert [l["step"] for l in train] == list(range(1, STEPS + 1))
    assert all(np.isfinite(l[k]) for l in train for k in ("train/loss", "train/osl", "train/del", "train/u_mape"))
    val = [l for l in lines if "val/loss" in l]
    assert len(val) == 1 and np.isfinite(val[0]["val/loss"])
    ck = torch.load(tmp_path / "run" / "checkpoints" / "best.ckpt", map_location="cpu", weights_only=False)
    assert ck["global_step"] == STEPS and "diffusion.proj_in.weight" in ck["state_dict"]


def test_fit_denoiser_resident_limit_is_checked(dev, tmp_path):
    cfg = _ragged_cfg(tmp_path, dev)
    cfg["data"].update(resident=True, resident_max_gb=1e-6)
    path = tmp_path / "small.yml"
    path.write_text(yaml.safe_dump(cfg))
    with pytest.raises(MemoryError, match="resident_max_gb"):
        fit_denoiser(str(path))
    cfg["data"].update(resident=False)
    path.write_text(yaml.safe_dump(cfg))
    with pytest.raises(ValueError, match="data.resident: true"):
        fit_denoiser(str(path))


def test_fit_style_resident(dev, tmp_path):
    """`fit-style` from a YAML with data.resident: the store holds s and labels only — the tree's h.npy files are gone — and four steps
    (three batches an epoch) log finite losses, validate on the resident validation table and write the checkpoint."""
    D = SO.STYLE_TINY
    data_dir = tmp_path / "data"
    write_synthetic_dataset(str(data_dir), n_maps=16, frames=8, a_dim=4, emb_dim=2, style_dim=D.style_dim, seed=3)
    for h in data_dir.glob("*/h.npy"):
        h.unlink()
    cfg = yaml.safe_load(open(DEFAULT_STYLE_CONFIG))
    cfg["model"].update(style_dim=D.style_dim, style_args=dict(label_features=D.label_features, h_dim=D.h_dim, depth=D.depth, expand=D.expand))
    cfg["data"].update(data_path=str(data_dir), batch_size=4, num_workers=0, shuffle_buffer_size=1, max_val_count=4, resident=True)
    cfg["trainer"].update(max_steps=4, log_every_n_steps=1, val_check_interval=3, default_root_dir=str(tmp_path / "run"), precision="32")
    path = tmp_path / "style.yml"
    path.write_text(yaml.safe_dump(cfg))
    module, trainer = fit_style(str(path))
    assert trainer.global_step == 4 and int(module.style_ema.n_averaged) == 4
    lines = [json.loads(l) for l in open(tmp_path / "run" / "metrics.jsonl")]
    train = [l for l in lines if "train/loss" in l]
    assert [l["step"] for l in train] == [1, 2, 3, 4] and all(np.isfinite(l["train/loss"]) for l in train)
    val = [l for l in lines if "val/energy_dist" in l]
    assert len(val) == 1 and np.isfinite(val[0]["val/energy_dist"])
    ck = torch.load(tmp_path / "run" / "checkpoints" / "best.ckpt", map_location="cpu", weights_only=False)
    assert ck["global_step"] == 3 and any(k.startswith("style_ema.module.") for k in ck["state_dict"])


def test_a_step_on_a_resident_batch_is_the_step_on_the_host_batch(dev, tmp_path):
    """The same maps through the resident feed and through load_latents + collate_ragged (what the host loader hands the trainer): the five
    tensors agree bit for bit, and with t / x0 pinned under OD_DETERMINISTIC so do the loss and every gradient."""
    frames = [70, 150, 96, 200, 33, 128, 90, 61]
    root = tmp_path / "data"
    write_synthetic_dataset(str(root), n_maps=len(frames), frames=frames, a_dim=16, emb_dim=6, style_dim=8, seed=1)
    torch.manual_seed(9)
    dm = ResidentLatentDataModule(batch_size=3, seq_len=None, num_workers=0, max_val_count=2, data_path=str(root), max_len=128, pad_multiple=64,
                                  batch_frames=384, bucket_pool=6, device=dev)
    feed = dm.train_dataloader()
    pb = max(feed.plan_epoch(), key=lambda p: len(p.maps))
    assert len(pb.maps) >= 2
    res = feed.gather(pb)
    samples = []
    for m, s0, n in zip(pb.maps.tolist(), pb.starts.tolist(), pb.lens.tolist()):
        h, z, s, labels = load_latents(dm.store.files[m])
        samples.append(LatentBatch(h[..., s0:s0 + n].clone(), z[..., s0:s0 + n].clone(), s, labels))
    host = collate_ragged(samples, 64)
    for k, a, b in zip(("h", "z", "s", "labels"), res[:4], host[:4]):
        assert a.shape == b.shape and torch.equal(a.cpu().view(torch.int32), b.view(torch.int32)), k
    assert torch.equal(res.lengths, host.lengths) and res.lengths.device.type == "cpu"

    d = O.Dims(emb_dim=6, a_dim=16, style_dim=8, global_cond_dim=32, backbone_dim=64, n_heads=2, head_dim=32, depth=1, expand=2, radius=2, u_head_dim=8)
    P = O.init_params(d, seed=41)
    for k in P:
        if any(z in k for z in ("ssg1.", "ssg2.", "proj_out.", "u_mod.")):
            P[k] = torch.randn(P[k].shape, generator=torch.Generator().manual_seed(len(k))) * 0.05
    B, Lpad = host.z.shape[0], host.z.shape[-1]
    gen = torch.Generator().manual_seed(42)
    t = (torch.rand(B, generator=gen) * 0.9 + 0.05).to(dev)
    x0 = torch.randn(B, 6, Lpad, generator=gen).to(dev)
    lens = [int(n) for n in host.lengths]
    runs = []
    try:
        det.force(True)
        for batch in (res, host):
            tr = make_trainer(d, P, dev)
            h, z, s, labels = (x.to(dev) for x in batch[:4])
            loss, logs = tr(tr.diffusion, h, z, s, labels, lengths=lens, t=t, x0=x0)
            loss.backward()
            runs.append((float(loss.detach()), {k: float(v) for k, v in logs.items()}, tr.diffusion.arena.grad.detach().cpu().clone()))
    finally:
        det.force(None)
    assert np.isfinite(runs[0][0]) and float(runs[0][2].abs().max()) > 0
    assert runs[0][0] == runs[1][0] and runs[0][1] == runs[1][1]
    assert torch.equal(runs[0][2].view(torch.int32), runs[1][2].view(torch.int32))
