"""`data.resident_val`: the held-out maps of fit-latent validated from a resident store, in ragged groups (resident.ResidentBeatmapValFeed,
LatentTrainer.validation_step on a data.RaggedBeatmapBatch), against the per-map step on the host loader's batch-1 tuples.

Rules:
  gathered batches   the whole-map and half batches equal the host path's padded tensors (read_spec / read_beatmap, .float(), pad_batch,
                     split_halves) bit for bit, zeros behind each map's padded length
  val/*              every map's 13 values equal the per-map step's bit for bit, the map's prior pinned to its two rows of the group's
  eval/*             every map's three values, and the epoch's dice, R^2 and score, within 1e-4 relative of the per-map path (each of the
                     five sums behind them is a sum of non-negative terms the kernel holds to 2e-5, and the score is a ratio of them)
  epoch means        the val/* means agree to 1e-12 relative: fp64 means of the same values in another order
  fit-latent         one validation record, best.ckpt at step 3, the host validation loader never called, eval/* as without the key
Emulator and MI355X (the `dev` fixture); fp32 and bf16.
"""
import json

import numpy as np
import pytest
import torch
import yaml

from osu_dreamer_amd.data import BeatmapDataModule, BeatmapDataset, RaggedBeatmapBatch, write_synthetic_beatmaps
from osu_dreamer_amd.fit import DEFAULT_LATENT_CONFIG, Trainer, build_beatmap_data, build_latent_from_config, fit_latent
from osu_dreamer_amd.latent_train import LOG_NAMES, LatentTrainer, split_halves
from osu_dreamer_amd.resident import ResidentBeatmapDataModule, ResidentBeatmapStore, ResidentBeatmapValFeed
from tools.gen_latent_train_golden import CASES, grad_weights, model_args, trainer_kwargs
from kernel_backend import bits, dev  # noqa: F401

FRAMES = (600, 180, 150, 131, 37)        # 180 needs no tail at either chunk size (multiples of 18 and of 8)
BUDGET = 400                             # padded frames: 600 alone (over the budget), then two groups of two
VAL_NAMES = tuple(f"val/{k}" for k in LOG_NAMES)
EVAL_NAMES = ("eval/cursor_px_mae", "eval/label_mae", "eval/z_var_min")
EPOCH_NAMES = ("eval/hit/dice", "eval/cursor/vel/r2", "eval/score")


def close(a, b, rel):
    a, b = float(a), float(b)
    return abs(a - b) <= rel * abs(b)


@pytest.fixture(scope="module")
def maps_dir(tmp_path_factory):
    d = tmp_path_factory.mktemp("val_maps")
    write_synthetic_beatmaps(str(d), n_mapsets=len(FRAMES), maps_per_set=1, frames=list(FRAMES), seed=11)
    return d


def make(name, device, bf16):
    c = CASES[name]
    tr = LatentTrainer(**trainer_kwargs(c, 0))
    tr.latent.load_state_dict(grad_weights(c))
    tr = tr.to(device).eval()
    if bf16:
        tr.latent.compute_dtype = torch.bfloat16
    return tr


def host_batch(f, device):
    """The host loader's batch-1 tuple of the map file f."""
    b = next(iter(BeatmapDataset([f.parent])))
    return tuple(t[None].to(device) for t in b)


@pytest.mark.parametrize("mode", ["fp32", "bf16"])
@pytest.mark.parametrize("name", ["tiny", "s4r1"])
def test_ragged_step_against_the_per_map_step(dev, maps_dir, name, mode):
    tr = make(name, dev, mode == "bf16")
    c2 = 2 * tr.latent.chunk_size
    store = ResidentBeatmapStore(sorted(maps_dir.iterdir()), dev)
    feed = ResidentBeatmapValFeed(store, c2, BUDGET)
    assert store.lengths.tolist() == list(FRAMES) and len(feed.short) == 0
    assert sorted(len(g) for g in feed.groups) == [1, 2, 2] and feed.groups[0].tolist() == [0]
    assert all(0.0 <= x < 0.5 for x in feed.padded_share())
    S = tr.latent.style_dim
    gen = torch.Generator().manual_seed(5)
    priors = [torch.randn(2 * len(g), S, generator=gen) for g in feed.groups]

    # ---- the groups, and their gathered tensors against the host path's
    tr.on_validation_epoch_start()
    got = {}
    for i, (grp, batch) in enumerate(zip(feed.groups, feed)):
        assert isinstance(batch, RaggedBeatmapBatch) and batch.lengths.tolist() == [FRAMES[m] for m in grp]
        batch = Trainer._to(None, batch, dev)
        logs = tr.validation_step(batch, i, prior=priors[i])
        for j, m in enumerate(grp.tolist()):
            got[m] = logs[j]
            audio, chart, _ = tr.pad_batch(host_batch(store.files[m], dev))
            P = audio.shape[-1]
            assert P == feed.plens[m] and P % c2 == 0
            for whole, halves, want in ((batch.audio, batch.audio_halves, audio), (batch.chart, batch.chart_halves, chart)):
                assert torch.equal(bits(whole[j, :, :P]), bits(want[0])), f"map {m}: the gathered whole map differs from the host path's"
                assert not bool(whole[j, :, P:].any()), f"map {m}: not zero behind the padded length"
                assert torch.equal(bits(halves[2 * j:2 * j + 2, :, :P // 2].contiguous()), bits(split_halves(want).contiguous())), f"map {m}: halves"
                assert not bool(halves[2 * j:2 * j + 2, :, P // 2:].any()), f"map {m}: halves not zero behind the padded length"
            assert torch.equal(batch.labels[j].cpu(), host_batch(store.files[m], "cpu")[2][0])
    assert len(tr._val) == len(FRAMES)
    epoch = {k: float(v) for k, v in tr.on_validation_epoch_end().items()}

    # ---- the per-map reference: the same trainer, map by map, each with its rows of its group's prior
    tr.on_validation_epoch_start()
    ref = {}
    for i, grp in enumerate(feed.groups):
        for j, m in enumerate(grp.tolist()):
            ref[m] = tr.validation_step(host_batch(store.files[m], dev), m, prior=priors[i][2 * j:2 * j + 2])
    ref_epoch = {k: float(v) for k, v in tr.on_validation_epoch_end().items()}

    for m in range(len(FRAMES)):
        for k in VAL_NAMES:
            a, b = got[m][k].float().cpu(), ref[m][k].float().cpu()
            assert torch.equal(bits(a.reshape(1)), bits(b.reshape(1))), f"{name} {mode} map {m} ({FRAMES[m]} frames) {k}: {float(a)!r} against the per-map {float(b)!r}"
        for k in EVAL_NAMES:
            print(f"map {m} {k}: {float(got[m][k]):.7g} (per map {float(ref[m][k]):.7g})")
            assert close(got[m][k], ref[m][k], 1e-4), (name, mode, m, k, float(got[m][k]), float(ref[m][k]))
    assert sorted(epoch) == sorted(ref_epoch)
    for k in EPOCH_NAMES + EVAL_NAMES:
        print(f"epoch {k}: {epoch[k]:.7g} (per map {ref_epoch[k]:.7g})")
        assert close(epoch[k], ref_epoch[k], 1e-4), (name, mode, k, epoch[k], ref_epoch[k])
    for k in VAL_NAMES:
        assert close(epoch[k], ref_epoch[k], 1e-12), (name, mode, k, epoch[k], ref_epoch[k])


def test_short_maps_take_the_per_map_step(dev, tmp_path):
    write_synthetic_beatmaps(str(tmp_path), n_mapsets=3, maps_per_set=1, frames=[40, 17, 18], seed=12)
    tr = make("tiny", dev, False)                       # 2 x chunk_size = 18: the 17-frame map is not grouped
    store = ResidentBeatmapStore(sorted(tmp_path.iterdir()), dev)
    feed = ResidentBeatmapValFeed(store, 18, None)
    assert [g.tolist() for g in feed.groups] == [[0, 2]] and feed.short.tolist() == [1] and len(feed) == 2
    batches = list(feed)
    assert isinstance(batches[0], RaggedBeatmapBatch) and not isinstance(batches[1], RaggedBeatmapBatch)
    want = host_batch(store.files[1], dev)
    assert all(torch.equal(bits(a), bits(b)) for a, b in zip(batches[1], want))
    tr.on_validation_epoch_start()
    for i, b in enumerate(batches):
        tr.validation_step(b, i)
    logs = tr.on_validation_epoch_end()
    assert len(tr._val) == 3 and all(np.isfinite(float(v)) for v in logs.values())


def test_the_trainer_refuses_another_pad_multiple(dev, maps_dir):
    tr = make("tiny", dev, False)
    feed = ResidentBeatmapValFeed(ResidentBeatmapStore(sorted(maps_dir.iterdir()), dev), 8, BUDGET)
    with pytest.raises(ValueError, match="2 x chunk_size"):
        tr.validation_step(next(iter(feed)), 0)


# ================================================================================================================ fit-latent
C = CASES["s4r1"]
SEQ, BATCH, STEPS = 4 * C.L, 3, 4


def _cfg(tmp_path, data_dir, run="run", **data):
    cfg = yaml.safe_load(open(DEFAULT_LATENT_CONFIG))
    a = model_args(C)
    cfg["model"].update(emb_dim=a["emb_dim"], style_dim=a["style_dim"], n_downs=a["n_downs"], stride=a["stride"], latent_args=a["args"],
                        schedule_args=dict(warmup_init=0.1, warmup_steps=4))
    cfg["data"].update(data_path=str(data_dir), batch_size=BATCH, seq_len=SEQ, num_workers=0, max_val_count=2, **data)
    cfg["trainer"].update(max_steps=STEPS, log_every_n_steps=1, val_check_interval=3, default_root_dir=str(tmp_path / run), precision="32")
    return cfg


def _run(tmp_path, data_dir, run, **data):
    path = tmp_path / f"{run}.yml"
    path.write_text(yaml.safe_dump(_cfg(tmp_path, data_dir, run, **data)))
    module, trainer = fit_latent(str(path))
    lines = [json.loads(l) for l in open(tmp_path / run / "metrics.jsonl")]
    return trainer, [l for l in lines if "eval/score" in l]


def test_fit_latent_resident_val(dev, tmp_path):
    data_dir = tmp_path / "data"
    write_synthetic_beatmaps(str(data_dir), n_mapsets=12, maps_per_set=1, frames=[150, 131] * 6, seed=3)
    calls = []
    host_val = BeatmapDataModule.val_dataloader

    def spy(self):
        calls.append(self)
        return host_val(self)
    BeatmapDataModule.val_dataloader = spy
    try:
        trainer, val = _run(tmp_path, data_dir, "on", resident=True, resident_val=True, resident_max_gb=0.01)
        assert calls == [], "the host validation loader was called"
        _, ref = _run(tmp_path, data_dir, "off", resident=True, resident_val=False)
        assert len(calls) == 1
    finally:
        BeatmapDataModule.val_dataloader = host_val
    assert trainer.global_step == STEPS
    assert len(val) == 1 and len(ref) == 1 and sorted(val[0]) == sorted(ref[0])
    assert np.isfinite(val[0]["val/loss"]) and np.isfinite(val[0]["eval/score"])
    assert torch.load(tmp_path / "on" / "checkpoints" / "best.ckpt", map_location="cpu", weights_only=False)["global_step"] == 3
    for k, v in val[0].items():
        if k.startswith("eval/"):
            print(f"{k}: {v:.7g} (host validation {ref[0][k]:.7g})")
            assert close(v, ref[0][k], 1e-4), (k, v, ref[0][k])
        elif k.startswith("val/"):              # these depend on the prior draw, which the two paths take in different shapes
            assert np.isfinite(v), k


def test_resident_val_needs_resident(tmp_path):
    cfg = _cfg(tmp_path, tmp_path / "data", resident_val=True)
    _, trainer = build_latent_from_config(cfg)
    with pytest.raises(ValueError, match="data.resident_val.*data.resident: true"):
        build_beatmap_data(dict(cfg["data"]), trainer, val_pad_multiple=8)
    with pytest.raises(ValueError, match="data.val_frame_budget.*data.resident_val: true"):
        build_beatmap_data(dict(cfg["data"], resident=True, resident_val=False, val_frame_budget=100), trainer, val_pad_multiple=8)


def test_resident_max_gb_bounds_both_stores(dev, tmp_path):
    data_dir = tmp_path / "data"
    write_synthetic_beatmaps(str(data_dir), n_mapsets=6, maps_per_set=1, frames=[150, 131] * 3, seed=3)
    cfg = _cfg(tmp_path, data_dir, resident=True, resident_val=True)
    _, trainer = build_latent_from_config(cfg)
    dm = build_beatmap_data(dict(cfg["data"]), trainer, val_pad_multiple=8)
    assert type(dm) is ResidentBeatmapDataModule and dm.val_feed is None          # built on first use
    feed = dm.val_dataloader()
    assert dm.val_dataloader() is feed and len(feed.store) >= 1
    train_bytes, val_bytes = dm.store.nbytes, feed.store.nbytes
    fits = build_beatmap_data(dict(cfg["data"], resident_max_gb=(train_bytes + val_bytes) / 2 ** 30), trainer, val_pad_multiple=8)
    assert len(fits.val_dataloader().store) == len(feed.store)
    tight = build_beatmap_data(dict(cfg["data"], resident_max_gb=(train_bytes + val_bytes - 1) / 2 ** 30), trainer, val_pad_multiple=8)
    made = []
    empty = torch.empty

    def spy(*a, **k):
        made.append(a)
        return empty(*a, **k)
    torch.empty = spy
    try:
        with pytest.raises(MemoryError, match="resident_max_gb"):
            tight.val_dataloader()
    finally:
        torch.empty = empty
    assert made == [] and tight.val_feed is None, "the store of the held-out maps was allocated before it was refused"
