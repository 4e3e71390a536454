"""`encode-latents`: a pre-processed dataset -> `<map>.latent.npz` {z, s, labels} + per-mapset `h.npy`, the files fit-denoiser's feeder
reads.  A synthetic dataset written with numpy (two mapsets, three maps, lengths not multiples of the chunk, one shorter than a chunk) is
encoded in batched varlen calls and checked against per-map encode_chart / per-mapset audio_encoder calls on the same weights; the
reference's skip rule and --force; the outputs load with data.load_latents and LatentDataModule iterates them.  The library function
runs through the `dev` fixture (emulator and MI355X), the command line on the MI355X."""
import os

import numpy as np
import pytest
import torch

from osu_dreamer_amd import data as D
from osu_dreamer_amd.encode_latents import encode_dataset, load_latent_ckpt, pack
from osu_dreamer_amd.ldm import pad_to_multiple
from kernel_backend import dev, rel_l2  # noqa: F401
from test_latent import load

MAPSETS = {"set_a": (58, ["101", "102"]), "set_b": (5, ["201"])}      # spec / chart frames, map ids


def write_dataset(root, seed=0):
    rng = np.random.default_rng(seed)
    for name, (L, maps) in MAPSETS.items():
        d = root / name
        d.mkdir(parents=True)
        np.save(d / "spec.npy", rng.integers(0, 256, (72, L), dtype=np.uint8))
        for mid in maps:
            xy_min = rng.uniform(-50, 0, (2, 1))
            xy_rng = rng.uniform(100, 500, (2, 1))
            with open(d / f"{mid}.map.npy", "wb") as f:
                np.savez(f, allow_pickle=False, hit=rng.integers(0, 256, (7, L), dtype=np.uint8),
                         xy=rng.integers(0, 65536, (2, L), dtype=np.uint16), xy_min=xy_min, xy_rng=xy_rng,
                         labels=rng.uniform(0, 10, 5))


def write_ckpt(path):
    fx, d, P = load("latent_tiny")
    hp = dict(emb_dim=d.emb_dim, style_dim=d.style_dim, n_downs=d.n_downs, stride=d.stride,
              latent_args=dict(h_dim=d.h_dim, ae_args=dict(n_layers=d.n_layers, expand=d.expand, radius=d.radius), style_head_dim=8,
                               style_heads=2))
    torch.save({"hyper_parameters": hp, "state_dict": {**{"latent." + k: v for k, v in P.items()}, "other.weight": torch.zeros(1)}},
               path)


def check_outputs(root, m):
    """Every output equals a per-map / per-mapset call of the reference's shape: fp32 1e-5 rel-L2 (the GEMMs may tile differently)."""
    c = m.chunk_size
    for name, (L, maps) in MAPSETS.items():
        d = root / name
        spec = D.read_spec(d / "spec.npy")
        assert spec.dtype == np.float64 and spec.max() <= 1.0
        a = pad_to_multiple(torch.from_numpy(spec).float()[None], c).to(next(m.parameters()).device)
        _, h_ref = m.audio_encoder(a)
        h = np.load(d / "h.npy")
        assert h.shape == (m.a_dim, -(-L // c)) and h.dtype == np.float32
        assert rel_l2(torch.from_numpy(h), h_ref[0]) <= 1e-5
        for mid in maps:
            chart, labels = D.read_beatmap(d / f"{mid}.map.npy")
            assert chart.shape == (9, L)
            x = pad_to_multiple(torch.from_numpy(chart).float()[None], c).to(a.device)
            z_ref, s_ref = m.encode_chart(x)
            with np.load(d / f"{mid}.latent.npz") as f:
                assert set(f.files) == {"z", "s", "labels"}
                assert f["z"].shape == (m.emb_dim, -(-L // c)) and f["s"].shape == (m.style_dim,)
                assert rel_l2(torch.from_numpy(f["z"]), z_ref[0]) <= 1e-5
                assert rel_l2(torch.from_numpy(f["s"]), s_ref[0]) <= 1e-5
                assert np.array_equal(f["labels"], labels)
            lb = D.load_latents(d / f"{mid}.latent.npz")
            assert lb.h.shape[-1] == lb.z.shape[-1]


def test_readers_match_disk_format(tmp_path):
    write_dataset(tmp_path)
    d = tmp_path / "set_a"
    raw = np.load(d / "spec.npy")
    assert np.array_equal(D.read_spec(d / "spec.npy"), raw.astype(float) / 255)
    chart, labels = D.read_beatmap(d / "101.map.npy")
    with np.load(d / "101.map.npy") as f:
        assert np.array_equal(chart[:7], f["hit"].astype(float) / 255)
        assert np.allclose(chart[7:], f["xy"].astype(float) / 65535 * f["xy_rng"] + f["xy_min"], rtol=0, atol=1e-12)
        assert np.array_equal(labels, f["labels"])


def test_pack_respects_budget():
    lens = [27, 9, 63, 45, 9]
    groups = pack(lens, 100)
    assert sorted(i for g in groups for i in g) == list(range(5))
    for g in groups:
        assert len(g) * max(lens[i] for i in g) <= 100 or len(g) == 1
    assert pack([200, 9], 100) == [[0], [1]]


def test_encode_dataset(dev, tmp_path):
    data = tmp_path / "data"
    write_dataset(data)
    ck = tmp_path / "latent.ckpt"
    write_ckpt(ck)
    m = load_latent_ckpt(str(ck), device=dev)
    assert encode_dataset(m, data, frame_budget=64) == (3, 2)        # a budget small enough to split the calls
    check_outputs(data, m)
    # skip rule: nothing to do
    stamp = {p: p.stat().st_mtime_ns for p in data.rglob("*.np*")}
    assert encode_dataset(m, data) == (0, 0)
    assert {p: p.stat().st_mtime_ns for p in data.rglob("*.np*")} == stamp
    # a missing latent: that map only, h.npy stays
    os.remove(data / "set_a" / "102.latent.npz")
    assert encode_dataset(m, data) == (1, 0)
    # a missing h.npy: its maps are redone and h written once
    os.remove(data / "set_a" / "h.npy")
    assert encode_dataset(m, data) == (2, 1)
    # --force: everything, one h per mapset
    assert encode_dataset(m, data, force=True) == (3, 2)
    check_outputs(data, m)
    # the feeder reads what was written
    dm = D.LatentDataModule(batch_size=1, seq_len=3, num_workers=0, max_val_count=1, max_val_frac=.5, data_path=str(data))
    batches = list(dm.train_dataloader())
    assert len(batches) >= 2
    h, z, s, labels = batches[0]
    assert h.shape == (1, m.a_dim, 3) and z.shape == (1, m.emb_dim, 3) and s.shape == (1, m.style_dim) and labels.shape == (1, 5)
    assert len(list(dm.val_dataloader())) == 1


def test_encode_dataset_empty(dev, tmp_path):
    ck = tmp_path / "latent.ckpt"
    write_ckpt(ck)
    m = load_latent_ckpt(str(ck), device=dev)
    (tmp_path / "empty").mkdir()
    with pytest.raises(RuntimeError):
        encode_dataset(m, tmp_path / "empty")


@pytest.mark.gpu
def test_encode_latents_cli(tmp_path):
    from osu_dreamer_amd import fit
    data = tmp_path / "data"
    write_dataset(data, seed=3)
    ck = tmp_path / "latent.ckpt"
    write_ckpt(ck)
    fit.main(["encode-latents", "--latent-ckpt-path", str(ck), "--data-dir", str(data), "--device", "cuda"])
    m = load_latent_ckpt(str(ck), device="cuda")
    check_outputs(data, m)
    stamp = {p: p.stat().st_mtime_ns for p in data.rglob("*.latent.npz")}
    fit.main(["encode-latents", "--latent-ckpt-path", str(ck), "--data-dir", str(data), "--device", "cuda"])
    assert {p: p.stat().st_mtime_ns for p in data.rglob("*.latent.npz")} == stamp
    fit.main(["encode-latents", "--latent-ckpt-path", str(ck), "--data-dir", str(data), "--device", "cuda", "--force",
              "--frame-budget", "64"])
    check_outputs(data, m)


def test_length_readers(tmp_path):
    write_dataset(tmp_path)
    for name, (L, maps) in MAPSETS.items():
        assert D.spec_length(tmp_path / name / "spec.npy") == L
        for mid in maps:
            assert D.beatmap_length(tmp_path / name / f"{mid}.map.npy") == L


def test_encode_dataset_reads_one_call_at_a_time(dev, tmp_path, monkeypatch):
    """Packing uses the arrays' headers only; each call's files are read when that call runs, and no earlier call's arrays are alive."""
    import weakref
    from osu_dreamer_amd import encode_latents as EL
    data = tmp_path / "data"
    write_dataset(data)
    ck = tmp_path / "latent.ckpt"
    write_ckpt(ck)
    m = load_latent_ckpt(str(ck), device=dev)
    live, reads, seen = [], {"spec": 0, "map": 0}, []

    def track(kind, fn):
        def wrapped(path):
            out = fn(path)
            reads[kind] += 1
            live.append(weakref.ref(out[0] if isinstance(out, tuple) else out))
            return out
        return wrapped
    monkeypatch.setattr(EL, "read_spec", track("spec", D.read_spec))
    monkeypatch.setattr(EL, "read_beatmap", track("map", D.read_beatmap))
    for name in ("_audio_encoder", "encode_chart"):
        fn = getattr(m, name)

        def call(x, lengths=None, _fn=fn):
            seen.append((dict(reads), sum(r() is not None for r in live), len(lengths)))
            return _fn(x, lengths)
        setattr(m, name, call)
    assert encode_dataset(m, data, frame_budget=64) == (3, 2)
    # frame budget 64 with chunk 9: every song / map is its own call (63 + 63 > 64 ... and 9 + 63 > 64 once sorted longest first)
    assert [s[2] for s in seen] == [1, 1, 1, 1, 1]
    assert [s[0]["spec"] for s in seen[:2]] == [1, 2] and [s[0]["map"] for s in seen[2:]] == [1, 2, 3]
    assert all(s[1] <= 1 for s in seen)                  # only the running call's array is alive
