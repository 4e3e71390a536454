"""The resident beatmap feed end to end (osu_dreamer_amd/resident.py), on the emulator and on the MI355X (the `dev` fixture): the store of
stored integers, the epoch plan with its flips, and od_feed_gather_quant — against data.read_spec / data.read_beatmap and the window and
flip code of BeatmapDataset.make_samples, bit for bit."""
import numpy as np
import pytest
import torch

from osu_dreamer_amd import resident
from osu_dreamer_amd.data import CURSOR_X, CURSOR_Y, read_beatmap, read_spec, write_synthetic_beatmaps
from osu_dreamer_amd.resident import (FLIP_X, FLIP_Y, EpochPlanner, ResidentBeatmapDataModule, ResidentBeatmapFeed, ResidentBeatmapStore)
from kernel_backend import dev  # noqa: F401

FRAMES, T = [300, 517, 130], 128


@pytest.fixture(scope="module")
def root(tmp_path_factory):
    d = tmp_path_factory.mktemp("beatmaps")
    write_synthetic_beatmaps(str(d), n_mapsets=3, maps_per_set=2, frames=FRAMES, seed=5)
    return d


@pytest.fixture(scope="module")
def host_maps(root):
    """What the host loader reads, once for the module: per map file (audio, chart, labels) as fp32 tensors (never modified)."""
    out = {}
    for f in sorted(root.glob("*/*.map.npy")):
        chart, labels = read_beatmap(f)
        out[f] = (torch.from_numpy(read_spec(f.parent / "spec.npy")).float(), torch.from_numpy(chart).float(),
                  torch.from_numpy(np.asarray(labels)).float())
    return out


def _feed(root, device, batch_size=2, seq_len=T, max_per_map=-1):
    store = ResidentBeatmapStore(sorted(root.iterdir()), device)
    return ResidentBeatmapFeed(store, EpochPlanner(store.lengths, batch_size, seq_len, max_per_map))


def _bits(t):
    return t.cpu().contiguous().view(torch.int32)


def test_batches_are_the_host_loaders_bit_for_bit(dev, root, host_maps):
    torch.manual_seed(11)
    feed = _feed(root, dev)
    st = feed.store
    assert [f.name for f in st.files] == ["0.map.npy", "1.map.npy"] * 3 and st.lengths.tolist() == [300, 300, 517, 517, 130, 130]
    rows, flips_seen = 0, set()
    for epoch in range(2):
        plan = feed.plan_epoch()
        per_map = np.bincount(np.concatenate([pb.maps for pb in plan]), minlength=6)
        assert (per_map[4:] <= 1).all() and (per_map[:2] <= 2).all() and (per_map[2:4] <= 4).all()     # drop_last may take one window away
        for pb in plan:
            assert len(pb.maps) == 2 and pb.Lpad == T and (pb.lens == T).all()
            batch = feed.gather(pb)
            assert batch.audio.shape == (2, 72, T) and batch.chart.shape == (2, 9, T) and batch.labels.shape == (2, 5)
            assert batch.audio.device.type == dev.type and batch.chart.is_contiguous()
            for i, (m, s0, fl) in enumerate(zip(pb.maps.tolist(), pb.starts.tolist(), pb.flips.tolist())):
                audio, chart, labels = host_maps[st.files[m]]
                window = chart[..., s0:s0 + T].clone()
                if fl & FLIP_X:
                    window[CURSOR_X].mul_(-1).add_(1)
                if fl & FLIP_Y:
                    window[CURSOR_Y].mul_(-1).add_(1)
                assert torch.equal(_bits(batch.audio[i]), _bits(audio[..., s0:s0 + T])), (epoch, m, s0)
                assert torch.equal(_bits(batch.chart[i]), _bits(window)), (epoch, m, s0, fl)
                assert torch.equal(_bits(batch.labels[i]), _bits(labels))
                rows += 1
                flips_seen.add(fl)
    assert rows >= 12 and len(flips_seen) >= 2


def test_window_rules(dev, root):
    """make_samples' rule on the chart lengths: the 130-frame maps yield exactly one window each (end = 3), a map shorter than seq_len
    none, `max_per_map` caps a map's windows and the last partial batch is dropped."""
    torch.manual_seed(12)
    feed = _feed(root, dev, batch_size=1)
    for _ in range(3):
        plan = feed.plan_epoch()
        per_map = np.bincount(np.concatenate([pb.maps for pb in plan]), minlength=6)
        assert per_map[4] == 1 and per_map[5] == 1
        assert all(1 <= per_map[i] <= 2 for i in (0, 1)) and all(3 <= per_map[i] <= 4 for i in (2, 3))
        for pb in plan:
            assert 0 <= pb.starts[0] and pb.starts[0] + T <= feed.store.lengths[pb.maps[0]]
        short = [pb for pb in plan if pb.maps[0] >= 4]
        assert all(0 <= pb.starts[0] < 3 for pb in short)
    # seq_len 200: the 130-frame maps are shorter than a window
    plan = ResidentBeatmapFeed(feed.store, EpochPlanner(feed.store.lengths, 1, 200)).plan_epoch()
    assert sorted(set(np.concatenate([pb.maps for pb in plan]).tolist())) == [0, 1, 2, 3]
    # max_per_map 1: six windows, one per map; batch_size 4 with drop_last: one batch of four
    plan = ResidentBeatmapFeed(feed.store, EpochPlanner(feed.store.lengths, 1, T, max_per_map=1)).plan_epoch()
    assert sorted(np.concatenate([pb.maps for pb in plan]).tolist()) == [0, 1, 2, 3, 4, 5]
    plan = ResidentBeatmapFeed(feed.store, EpochPlanner(feed.store.lengths, 4, T, max_per_map=1)).plan_epoch()
    assert len(plan) == 1 and len(plan[0].maps) == 4 and len(set(plan[0].maps.tolist())) == 4 and len(plan[0].flips) == 4
    plan = ResidentBeatmapFeed(feed.store, EpochPlanner(feed.store.lengths, 4, T, max_per_map=2)).plan_epoch()
    assert len(plan) == 2 and np.bincount(np.concatenate([pb.maps for pb in plan]), minlength=6).max() <= 2


def test_maps_of_a_mapset_share_one_spectrogram(dev, root):
    st = ResidentBeatmapStore(sorted(root.iterdir()), dev)
    assert st.spec_base[0] == st.spec_base[1] and st.spec_base[2] == st.spec_base[3] and st.spec_base[4] == st.spec_base[5]
    assert len(set(st.spec_base.tolist())) == 3 and st.spec_stride.tolist() == [300, 300, 517, 517, 130, 130]
    assert len(set(st.hit_base.tolist())) == 6 and len(set(st.xy_base.tolist())) == 6
    # one copy of each spectrogram, 7 + 4 bytes per chart frame, at most 3 bytes of alignment in front of each xy
    need = 72 * sum(FRAMES) + 11 * 2 * sum(FRAMES)
    assert st.data.dtype == torch.uint8 and need <= st.data.numel() <= need + 3 * 6
    assert st.xy_rng.dtype == np.float64 and st.xy_rng.shape == (6, 2) and st.xy_min.shape == (6, 2)
    assert st.labels.dtype == torch.float32 and st.labels.shape == (6, 5) and st.labels.device.type == dev.type
    # as stored: the spectrogram's bytes are the file's
    spec = np.load(st.files[2].parent / "spec.npy")
    b = int(st.spec_base[2])
    assert np.array_equal(st.data[b:b + spec.size].cpu().numpy(), spec.reshape(-1))


def test_flips_are_fair_coins(dev, root):
    """4096 planned windows: all four flip pairs occur and each flip's frequency lies in 0.5 +- 0.05 (6.4 sigma of a fair coin over 4096
    draws, sigma = 0.0078); the seed is fixed."""
    torch.manual_seed(13)
    st = ResidentBeatmapStore(sorted(root.iterdir())[2:], dev)          # planning reads the planner's lengths only
    feed = ResidentBeatmapFeed(st, EpochPlanner(np.full(4096, T + 40), 64, T, max_per_map=1))
    plan = feed.plan_epoch()
    flips = np.concatenate([pb.flips for pb in plan])
    assert len(flips) == 4096 and flips.dtype == np.int32 and sorted(set(flips.tolist())) == [0, 1, 2, 3]
    fx, fy = float((flips & FLIP_X).astype(bool).mean()), float((flips & FLIP_Y).astype(bool).mean())
    assert abs(fx - 0.5) <= 0.05 and abs(fy - 0.5) <= 0.05, (fx, fy)
    both = float((flips == 3).mean())
    assert abs(both - 0.25) <= 0.05, both                      # the two flips of a window are drawn independently


def test_same_seed_same_plan(dev, root):
    def epochs(seed):
        torch.manual_seed(seed)
        feed = _feed(root, dev)
        return [[(pb.maps.tolist(), pb.starts.tolist(), pb.flips.tolist()) for pb in feed.plan_epoch()] for _ in range(2)]
    a, b = epochs(21), epochs(21)
    assert a == b and a[0] != a[1]
    assert epochs(22)[0] != a[0]


def test_data_module(dev, root):
    """The constructor keys of BeatmapDataModule plus device / resident_max_gb: the host module's hold-out, the store over the training
    mapsets only, validation from the host loader."""
    dm = ResidentBeatmapDataModule(batch_size=2, seq_len=T, num_workers=0, max_val_count=2, max_val_frac=0.4, data_path=str(root), max_per_map=1,
                                   device=dev, resident_max_gb=0.01)
    assert [m.name for m in dm.host.val_set.mapsets] == ["0000"] and [f.parent.name for f in dm.store.files] == ["0001", "0001", "0002", "0002"]
    batches = list(dm.train_dataloader())
    assert len(batches) == 2 and all(b.audio.shape == (2, 72, T) for b in batches)
    val = list(dm.val_dataloader())
    assert len(val) == 2 and val[0][0].shape == (1, 72, 300) and val[0][0].device.type == "cpu"
    with pytest.raises(ValueError, match="seq_len"):
        ResidentBeatmapDataModule(batch_size=2, seq_len=None, data_path=str(root), max_val_count=2, max_val_frac=0.4, device=dev)


def test_max_bytes_refusal_allocates_nothing(dev, root, monkeypatch):
    def boom(*a, **k):
        raise AssertionError("allocated before the size check")
    monkeypatch.setattr(resident.torch, "empty", boom)
    monkeypatch.setattr(resident.np, "load", boom)
    with pytest.raises(MemoryError, match=r"resident_max_gb"):
        ResidentBeatmapStore(sorted(root.iterdir()), dev, max_bytes=10_000)


def _rewrite(path, **changes):
    with np.load(path) as d:
        arrays = {k: d[k] for k in d.files}
    arrays.update({k: fn(arrays[k]) for k, fn in changes.items()})
    with open(path, "wb") as f:
        np.savez(f, **arrays)


def test_dtype_and_length_refusals(dev, tmp_path):
    write_synthetic_beatmaps(str(tmp_path), n_mapsets=2, maps_per_set=1, frames=[140, 150], seed=6)
    sets = sorted(tmp_path.iterdir())
    ResidentBeatmapStore(sets, dev)                               # as written: accepted
    spec = sets[0] / "spec.npy"
    good = np.load(spec)
    np.save(spec, good.astype(np.uint16))
    with pytest.raises(ValueError, match=r"0000/spec\.npy.*uint16"):
        ResidentBeatmapStore(sets, dev)
    np.save(spec, good[:, :139])                                  # one frame shorter than its map
    with pytest.raises(ValueError, match=r"0000/spec\.npy.*shorter"):
        ResidentBeatmapStore(sets, dev)
    np.save(spec, good)
    _rewrite(sets[1] / "0.map.npy", hit=lambda a: a.astype(np.uint16))
    with pytest.raises(ValueError, match=r"0001/0\.map\.npy.*hit is uint16"):
        ResidentBeatmapStore(sets, dev)
    _rewrite(sets[1] / "0.map.npy", hit=lambda a: a.astype(np.uint8), xy=lambda a: a.astype(np.float32))
    with pytest.raises(ValueError, match=r"0001/0\.map\.npy.*xy is float32"):
        ResidentBeatmapStore(sets, dev)
