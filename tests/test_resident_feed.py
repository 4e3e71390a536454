"""The resident feed end to end (osu_dreamer_amd/resident.py), on the emulator and on the MI355X (the `dev` fixture): store, plan, od_feed_gather.

A synthetic tree with a_dim 4, emb_dim 2, maps of 8 .. 200 frames and one mapset with two maps sharing its h.npy.  Every batch the feed yields
must equal — bit for bit, it is a copy — what the host loader's own functions build for the maps and windows the plan names: the plain
stack of `load_latents` slices for fixed windows, `collate_ragged` of them for whole maps.
"""
import numpy as np
import pytest
import torch

from osu_dreamer_amd import resident
from osu_dreamer_amd.data import LatentBatch, RaggedLatentBatch, collate_ragged, load_latents, write_synthetic_dataset
from osu_dreamer_amd.resident import STYLE_FIELDS, ResidentLatentDataModule, ResidentLatentStore
from kernel_backend import dev  # noqa: F401

FRAMES = [8, 70, 131, 40, 9, 200]
A, E, S = 4, 2, 8


def _tree(root, seed=5):
    write_synthetic_dataset(str(root), n_maps=len(FRAMES), frames=FRAMES, a_dim=A, emb_dim=E, style_dim=S, seed=seed)
    rng = np.random.default_rng(seed + 1)                   # a second difficulty in mapset 0002: shorter than the mapset's h (131 frames)
    np.savez(root / "0002" / "1.latent.npz", z=rng.standard_normal((E, 120)).astype(np.float32),
             s=rng.standard_normal(S).astype(np.float32), labels=(rng.random(5) * 10).astype(np.float32))
    return root


@pytest.fixture(scope="module")
def tree(tmp_path_factory):
    return _tree(tmp_path_factory.mktemp("resident"))


def _module(root, device, **kw):
    # max_val_count 1: mapset 0000 (one map of 8 frames) is held out, 0001 .. 0005 train: six maps, two of them in 0002
    args = dict(batch_size=2, seq_len=None, num_workers=0, max_val_count=1, max_val_frac=.3, data_path=str(root), device=device)
    args.update(kw)
    return ResidentLatentDataModule(**args)


def _same(a, b, what):
    assert a.shape == b.shape and a.dtype == b.dtype, (what, a.shape, b.shape)
    assert torch.equal(a.cpu().view(torch.int32), b.view(torch.int32)), what


def _check_epoch(dm, pad_multiple=64):
    feed = dm.train_dataloader()
    plan = feed.plan_epoch()
    assert plan
    for pb in plan:
        got = feed.gather(pb)
        samples = []
        for m, s0, n in zip(pb.maps.tolist(), pb.starts.tolist(), pb.lens.tolist()):
            h, z, s, labels = load_latents(dm.store.files[m])
            samples.append(LatentBatch(h[..., s0:s0 + n].clone(), z[..., s0:s0 + n].clone(), s, labels))
        if dm.ragged:
            want = collate_ragged(samples, pad_multiple)
            assert isinstance(got, RaggedLatentBatch) and got.lengths.device.type == "cpu" and got.lengths.dtype == torch.int64
            assert torch.equal(got.lengths, want.lengths) and got.h.shape[-1] == pb.Lpad
        else:
            want = LatentBatch(*(torch.stack(t) for t in zip(*samples)))
            assert len(got) == 4
        for k, g, w in zip("hzsl", got[:4], want[:4]):
            assert g.device.type == dm.device.type
            _same(g, w, (k, pb))
    return plan


def test_store_layout(dev, tree):
    dm = _module(tree, dev)
    st = dm.store
    assert [f.parent.name + "/" + f.name for f in st.files] == ["0001/0.latent.npz", "0002/0.latent.npz", "0002/1.latent.npz", "0003/0.latent.npz",
                                                                "0004/0.latent.npz", "0005/0.latent.npz"]
    assert st.lengths.tolist() == [70, 131, 120, 40, 9, 200]
    assert st.h_base[1] == st.h_base[2] and st.h_stride[1] == st.h_stride[2] == 131          # one h for the mapset's two maps
    assert st.data.numel() == A * (70 + 131 + 40 + 9 + 200) + E * (70 + 131 + 120 + 40 + 9 + 200)
    assert st.nbytes == 4 * (st.data.numel() + 6 * (S + 5)) and st.s.shape == (6, S) and st.labels.shape == (6, 5)


def test_fixed_windows_equal_the_stacked_slices(dev, tree):
    for seq_len, per_map in ((8, -1), (37, 2), (9, 1)):
        torch.manual_seed(seq_len)
        dm = _module(tree, dev, seq_len=seq_len, batch_size=3, max_per_map=per_map)
        plan = _check_epoch(dm)
        assert all(len(pb.maps) == 3 for pb in plan)
    # both maps of mapset 0002 were drawn from (the shared h at two maps' windows)
    assert {1, 2} <= set(np.concatenate([pb.maps for pb in plan]).tolist())


def test_whole_map_chunks_equal_collate_ragged(dev, tree):
    torch.manual_seed(1)
    dm = _module(tree, dev, batch_size=2, max_len=100, pad_multiple=64)
    plan = _check_epoch(dm)
    assert len(plan) == 3 and sorted(np.concatenate([pb.maps for pb in plan]).tolist()) == list(range(6))
    assert max(int(pb.lens.max()) for pb in plan) == 100
    _check_epoch(_module(tree, dev, batch_size=3, pad_multiple=5), pad_multiple=5)      # Lpad no multiple of four: the dword path alone


def test_frame_budget_batches_equal_collate_ragged(dev, tree):
    torch.manual_seed(2)
    dm = _module(tree, dev, batch_size=4, max_len=128, pad_multiple=64, batch_frames=256, bucket_pool=4)
    plan = _check_epoch(dm)
    assert sorted(np.concatenate([pb.maps for pb in plan]).tolist()) == list(range(6))      # no map dropped, the partial pool included
    assert all(len(pb.maps) * pb.Lpad <= 256 and len(pb.maps) <= 4 for pb in plan)


def test_epochs_differ_and_follow_the_seed(dev, tree):
    def two_epochs():
        torch.manual_seed(3)
        feed = _module(tree, dev, seq_len=8, batch_size=2, max_per_map=1).train_dataloader()
        return [[(b.h.cpu(), b.s.cpu()) for b in feed] for _ in range(2)]
    a, b = two_epochs(), two_epochs()
    assert len(a[0]) == 3 and len(a[1]) == 3                # six maps, one window each (mapset 0000 is held out), batches of two
    flat = lambda ep: torch.cat([h.flatten() for h, _ in ep])        # noqa: E731
    assert torch.equal(flat(a[0]), flat(b[0])) and torch.equal(flat(a[1]), flat(b[1]))
    assert not torch.equal(flat(a[0]), flat(a[1]))


def test_style_store_never_opens_h(dev, tmp_path):
    root = _tree(tmp_path / "style")
    want = {f: load_latents(f) for f in sorted(root.glob("*/*.latent.npz"))}
    for h in root.glob("*/h.npy"):
        h.unlink()
    torch.manual_seed(4)
    dm = _module(root, dev, seq_len=1, batch_size=3, max_per_map=1, fields=STYLE_FIELDS)
    assert not dm.store.has_frames and dm.store.data.numel() == 1
    feed = dm.train_dataloader()
    plan = feed.plan_epoch()
    assert len(plan) == 2 and sorted(np.concatenate([pb.maps for pb in plan]).tolist()) == list(range(6))
    for pb in plan:
        h, z, s, labels = feed.gather(pb)
        assert h.shape == (3, 0, 1) and z.shape == (3, 0, 1)
        _same(s, torch.stack([want[dm.store.files[m]].s for m in pb.maps.tolist()]), "s")
        _same(labels, torch.stack([want[dm.store.files[m]].labels for m in pb.maps.tolist()]), "labels")
    val = list(dm.val_dataloader())
    assert len(val) == 1 and val[0][0].numel() == 0 and val[0][1].numel() == 0
    f0 = root / "0000" / "0.latent.npz"
    _same(val[0][2], want[f0].s[None], "val s")
    _same(val[0][3], want[f0].labels[None], "val labels")


def test_a_store_over_the_limit_raises_before_it_allocates(dev, tree, monkeypatch):
    need = _module(tree, dev).store.nbytes

    def no_alloc(*a, **k):
        raise AssertionError("allocated before the size check")
    monkeypatch.setattr(resident.torch, "empty", no_alloc)
    monkeypatch.setattr(resident.np, "load", no_alloc)                 # nor is any array read
    with pytest.raises(MemoryError, match=rf"needs {need} bytes.*limit of {need - 1} bytes"):
        ResidentLatentStore(sorted(tree.iterdir())[1:], dev, max_bytes=need - 1)
    with pytest.raises(MemoryError, match="resident_max_gb"):
        _module(tree, dev, resident_max_gb=1e-7)
    monkeypatch.undo()
    assert ResidentLatentStore(sorted(tree.iterdir())[1:], dev, max_bytes=need).nbytes == need


def test_the_denoiser_validates_on_the_host_loader(dev, tree):
    val = list(_module(tree, dev).val_dataloader())
    assert len(val) == 1 and val[0][1].shape == (1, E, 8) and val[0][0].device.type == "cpu"


@pytest.mark.parametrize("B", [1, 3])
def test_packed_descriptors_are_views_of_one_block(B):
    """pack_descriptors, host only: every column comes back as a view of ONE block (one copy took them all), in the order given, with its
    values and shape; the fp64 views start on 8-byte boundaries — the int32 columns lie behind every 8-byte one — also at an odd B."""
    rng = np.random.default_rng(B)
    i64 = [rng.integers(-2 ** 40, 2 ** 40, B) for _ in range(3)]
    f64 = [rng.standard_normal((B, 2)) for _ in range(2)]
    i32 = [rng.integers(0, 2 ** 20, B) for _ in range(2)]               # int64 host columns, as a plan's lens are
    views = resident.pack_descriptors(torch.device("cpu"), False, i64=i64, f64=f64, i32=i32)
    assert len(views) == 7 and len({v.untyped_storage().data_ptr() for v in views}) == 1
    assert views[0].untyped_storage().nbytes() == 8 * (3 * B + 4 * B + (2 * B + 1) // 2)
    for v, c, dt in zip(views, i64 + f64 + i32, [torch.int64] * 3 + [torch.float64] * 2 + [torch.int32] * 2):
        assert v.dtype == dt and tuple(v.shape) == c.shape and np.array_equal(v.numpy(), c.astype(v.numpy().dtype)), (dt, c)
    assert all(v.data_ptr() % 8 == 0 for v in views[:5])
    assert [v.data_ptr() for v in views] == sorted(v.data_ptr() for v in views)
    only, = resident.pack_descriptors(torch.device("cpu"), False, i64=i64[:1])      # the style feed's one column
    assert only.dtype == torch.int64 and np.array_equal(only.numpy(), i64[0])
