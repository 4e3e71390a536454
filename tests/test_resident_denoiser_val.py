"""`data.resident_val` of fit-denoiser: the held-out maps validated from a resident store, in groups of whole maps
(resident.ResidentLatentValFeed, DiffusionTrainer.validation_step on a data.RaggedLatentValBatch, fit.Trainer.validate), against the per-map
step on the host loader's batch-1 tuples.

Six maps of 131, 64, 9, 8, 7 and 131 latent frames, val_batches = 8, pad_multiple = 64: segments of 16, 8, 1, 1, 0 and 16 frames.

Rules:
  gathered groups    row 8 g + j of a group equals, bit for bit, segment j of map g as validation_step cuts it from the host loader's tensors;
                     zeros behind the segment; offs, lengths, s and labels are the maps'; every map once per epoch; a budget below one map
                     still yields it, alone
  the short map      7 frames have no frame per segment: that map alone (1 of 6) is not grouped and follows the groups as the host loader's
                     batch-1 tuple, bit for bit.  validation_step has never accepted such a map (od_rope_table refuses zero frames), from
                     either loader: that is asserted as it stands, and the shell tests hold out the four maps before it
  per map            with t and x0 pinned, a grouped map's loss / osl / del / u_mape against validation_step on that map alone (its eight t,
                     its x0 rows cut to its segment): 1e-5 relative in fp32, 1e-4 in bf16 — the bounds tests/test_ragged_train.py holds the
                     ragged loss terms to against single-song steps (measured there at 2e-7 and 4e-6; measured here, worst value of
                     any map: 2.1e-7 and 1.6e-7 on the MI355X, 7.9e-8 and 1.2e-7 on the emulator)
  the shell          Trainer.validate over both data modules, draws pinned per map: val/* within the same bounds, the same maps counted;
                     limit_val_batches = 3 validates the host loader's first three maps; one host read per group
  off                without the keys val_dataloader() is the host loader's
  refusals           resident_val without resident, a budget without resident_val, resident_val on a style-only store, and two stores over
                     resident_max_gb (before anything is allocated)
  fit-denoiser       a few steps with resident_val: finite metrics, best.ckpt on val/loss, as many maps validated as without the key
Emulator and MI355X (the `dev` fixture).
"""
import copy
import json

import numpy as np
import pytest
import torch
import yaml
from torch.utils.data import DataLoader

from oracle import denoiser_oracle as O
from osu_dreamer_amd import _lib
from osu_dreamer_amd.data import LatentDataModule, RaggedLatentValBatch, load_latents, write_synthetic_dataset
from osu_dreamer_amd.fit import Trainer, build_latent_data, fit_denoiser
from osu_dreamer_amd.resident import ResidentLatentDataModule, ResidentLatentStore, ResidentLatentValFeed
from osu_dreamer_amd.train import VAL_LOG_NAMES, DiffusionTrainer
from kernel_backend import bits, dev  # noqa: F401
from test_model_parity import make_trainer
from test_ragged_train import _dims, _ragged_cfg

FRAMES = [131, 64, 9, 8, 7, 131]
VB, PAD = 8, 64
SEGS = [n // VB for n in FRAMES]
BOUND = {"fp32": 1e-5, "bf16": 1e-4}
D = _dims(32, 2)


@pytest.fixture(scope="module")
def data_dir(tmp_path_factory):
    d = tmp_path_factory.mktemp("denoiser_val_maps")
    write_synthetic_dataset(str(d), n_maps=len(FRAMES), frames=FRAMES, a_dim=D.a_dim, emb_dim=D.emb_dim, style_dim=D.style_dim, seed=21)
    return d


def make(device, mode="fp32"):
    P = O.init_params(D, seed=91)
    for k in P:                                   # (the reference zero-initialises these: un-zero them so every layer shapes the output)
        if any(z in k for z in ("ssg1.", "ssg2.", "proj_out.", "u_mod.")):
            P[k] = torch.randn(P[k].shape, generator=torch.Generator().manual_seed(len(k))) * 0.05
    tr = make_trainer(D, P, device)
    tr.val_batches = VB
    if mode == "bf16":
        tr.diffusion.compute_dtype = tr.diffusion_ema.module.compute_dtype = torch.bfloat16
    return tr.eval()


def host_tuple(f, device):
    """The host loader's batch-1 tuple of the latent file f."""
    return tuple(t[None].to(device) for t in load_latents(f))


def cut(x, seg):
    """(1, C, L) -> (VB, C, seg), as DiffusionTrainer.validation_step cuts a map."""
    return x[..., :VB * seg].reshape(x.size(1), VB, seg).permute(1, 0, 2).contiguous()


def draws(device, seed=5):
    """Per map of FRAMES: its eight t and its x0 rows at the padded width (a group's padding of x0 is never read)."""
    gen = torch.Generator().manual_seed(seed)
    T = [(torch.rand(VB, generator=gen) * 0.9 + 0.05).to(device) for _ in FRAMES]
    X0 = [torch.randn(VB, D.emb_dim, PAD, generator=gen).to(device) for _ in FRAMES]
    return T, X0


# ================================================================================================================ the feed
def test_groups_hold_the_segments_validation_step_cuts(dev, data_dir):
    store = ResidentLatentStore(sorted(data_dir.iterdir()), dev)
    assert store.lengths.tolist() == FRAMES
    feed = ResidentLatentValFeed(store, VB, PAD, 1024)           # a map pads to 8 x 64 frames: two maps a group
    assert [g.tolist() for g in feed.groups] == [[0, 1], [2, 3], [5]] and feed.short.tolist() == [4] and len(feed) == 4
    assert sorted(m for g in feed.groups for m in g.tolist()) + feed.short.tolist() == [0, 1, 2, 3, 5, 4]
    assert all(0.0 <= x < 1.0 for x in feed.padded_share()) and feed.padded_share()[0] == 1.0 - (16 + 8) / 128
    batches = list(feed)
    assert len(batches) == 4
    for grp, batch in zip(feed.groups, batches):
        assert isinstance(batch, RaggedLatentValBatch)
        G = len(grp)
        assert batch.h.shape == (VB * G, D.a_dim, PAD) and batch.z.shape == (VB * G, D.emb_dim, PAD)
        assert batch.offs.tolist() == list(range(0, VB * G + 1, VB)) and batch.offs.device.type == "cpu"
        assert batch.lengths.tolist() == [SEGS[m] for m in grp.tolist() for _ in range(VB)] and batch.lengths.device.type == "cpu"
        for j, m in enumerate(grp.tolist()):
            h, z, s, labels = host_tuple(store.files[m], dev)
            seg, rows = SEGS[m], slice(VB * j, VB * (j + 1))
            for got, want, what in ((batch.h, h, "h"), (batch.z, z, "z")):
                assert torch.equal(bits(got[rows, :, :seg].contiguous()), bits(cut(want, seg))), f"map {m}: {what} differs from the host path's segments"
                assert not bool(got[rows, :, seg:].any()), f"map {m}: {what} is not zero behind its segment"
            assert torch.equal(bits(batch.s[j]), bits(s[0])) and torch.equal(bits(batch.labels[j]), bits(labels[0]))
    # the 7-frame map: the host loader's tuple, after the groups
    short = batches[-1]
    assert not isinstance(short, RaggedLatentValBatch) and len(short) == 4
    for a, b in zip(short, host_tuple(store.files[4], dev)):
        assert a.shape == b.shape and torch.equal(bits(a.contiguous()), bits(b))
    # re-iterable, and the same every epoch
    again = list(feed)
    assert all(torch.equal(bits(a.z), bits(b.z)) for a, b in zip(batches[:3], again[:3]))


def test_budget_and_limit(dev, data_dir):
    store = ResidentLatentStore(sorted(data_dir.iterdir()), dev)
    one = ResidentLatentValFeed(store, VB, PAD)                  # the default budget: one group
    assert [g.tolist() for g in one.groups] == [[0, 1, 2, 3, 5]] and one.short.tolist() == [4]
    tight = ResidentLatentValFeed(store, VB, PAD, 100)           # below one map's 512 padded frames: every map still comes, alone
    assert [g.tolist() for g in tight.groups] == [[0], [1], [2], [3], [5]]
    assert next(iter(tight)).z.shape == (VB, D.emb_dim, PAD)
    assert one.limit(3) is one and [g.tolist() for g in one.groups] == [[0, 1, 2]] and one.short.tolist() == []
    assert [g.tolist() for g in one.limit(5).groups] == [[0, 1, 2, 3]] and one.short.tolist() == [4]
    assert [g.tolist() for g in one.limit(None).groups] == [[0, 1, 2, 3, 5]]
    with pytest.raises(ValueError, match="val_frame_budget"):
        ResidentLatentValFeed(store, VB, PAD, 0)


def test_a_map_without_a_frame_per_segment_is_refused_as_ever(dev, data_dir):
    """Seven frames in eight segments: validation_step refuses the map (no kernel runs on zero frames), and it refuses the resident feed's
    tuple as it refuses the host loader's."""
    tr = make(dev)
    store = ResidentLatentStore(sorted(data_dir.iterdir()), dev)
    feed = ResidentLatentValFeed(store, VB, PAD)
    for batch in (feed.gather_one(4), host_tuple(store.files[4], dev)):
        with pytest.raises(_lib.HipKernelError):
            tr.validation_step(batch, 0)


# ================================================================================================================ per map
@pytest.mark.parametrize("mode", ["fp32", "bf16"])
def test_a_grouped_map_against_its_own_step(dev, data_dir, mode):
    tr = make(dev, mode)
    store = ResidentLatentStore(sorted(data_dir.iterdir()), dev)
    feed = ResidentLatentValFeed(store, VB, PAD, 1536)           # three maps a group
    assert [g.tolist() for g in feed.groups] == [[0, 1, 2], [3, 5]]
    T, X0 = draws(dev)
    worst = 0.0
    for i, (grp, batch) in enumerate(zip(feed.groups, feed)):
        maps = grp.tolist()
        logs = tr.validation_step(batch, i, t=torch.cat([T[m] for m in maps]), x0=torch.cat([X0[m] for m in maps]))
        assert list(logs) == list(VAL_LOG_NAMES) and all(v.shape == (len(maps),) and v.device.type == dev.type for v in logs.values())
        for j, m in enumerate(maps):
            alone = tr.validation_step(host_tuple(store.files[m], dev), m, t=T[m], x0=X0[m][..., :SEGS[m]].contiguous())
            for k in VAL_LOG_NAMES:
                a, b = float(logs[k][j]), float(alone[k])
                rel = abs(a - b) / abs(b)
                worst = max(worst, rel)
                print(f"{mode} map {m} ({FRAMES[m]} frames) {k}: grouped {a:.8g}, alone {b:.8g}, relative {rel:.2e}")
                assert np.isfinite(a) and rel <= BOUND[mode], (mode, m, k, a, b)
    print(f"{mode}: worst relative distance {worst:.2e} (bound {BOUND[mode]:.0e})")


def test_the_group_draws_t_per_map(dev, data_dir):
    """Unpinned: finite values, and t stratified per map — every map's eight t fall one in each eighth of the logit-normal's quantiles."""
    tr = make(dev)
    store = ResidentLatentStore(sorted(data_dir.iterdir()), dev)
    batch = next(iter(ResidentLatentValFeed(store, VB, PAD)))
    seen = []
    fwd = torch.special.ndtri

    def spy(u01):
        seen.append(u01.detach().cpu())
        return fwd(u01)
    torch.special.ndtri = spy
    try:
        torch.manual_seed(3)
        logs = tr.validation_step(batch, 0)
    finally:
        torch.special.ndtri = fwd
    assert all(bool(torch.isfinite(v).all()) for v in logs.values())
    u01 = seen[0].reshape(-1, VB)
    assert u01.shape == (5, VB)
    assert all(sorted((row * VB).floor().int().tolist()) == list(range(VB)) for row in u01)


# ================================================================================================================ the shell
DATA = dict(batch_size=2, seq_len=None, num_workers=0, max_val_count=4, max_val_frac=.9, pad_multiple=PAD)     # held out: maps 0 .. 3


class Counted(torch.Tensor):
    """A tensor whose host reads are counted (and whose results are plain tensors again)."""
    reads = []

    @staticmethod
    def __new__(cls, t):
        return torch.Tensor._make_subclass(cls, t)

    def cpu(self, *a, **k):
        Counted.reads.append("cpu")
        return super().cpu(*a, **k).as_subclass(torch.Tensor)

    def item(self):
        Counted.reads.append("item")
        return super().item()

    def tolist(self):
        Counted.reads.append("tolist")
        return super().tolist()

    def __float__(self):
        Counted.reads.append("float")
        return float(self.as_subclass(torch.Tensor))


def pinned(tr, dm, seen, device):
    """tr.validation_step with every map's draws pinned (draws()), whichever loader hands the map over; `seen` collects the maps."""
    T, X0 = draws(device)
    step = DiffusionTrainer.validation_step

    def validation_step(batch, batch_idx):
        if isinstance(batch, RaggedLatentValBatch):
            maps = dm.val_feed.groups[batch_idx].tolist()
            logs = step(tr, batch, batch_idx, t=torch.cat([T[m] for m in maps]), x0=torch.cat([X0[m] for m in maps]))
        else:
            maps = [batch_idx]                                    # the host loader: one map a batch, in order
            logs = step(tr, batch, batch_idx, t=T[batch_idx], x0=X0[batch_idx][..., :SEGS[batch_idx]].contiguous())
        seen.extend(maps)
        return {k: Counted(v) for k, v in logs.items()}
    return validation_step


@pytest.mark.parametrize("mode", ["fp32", "bf16"])
def test_validate_over_both_data_modules(dev, data_dir, tmp_path, mode):
    tr = make(dev, mode)
    host = LatentDataModule(data_path=str(data_dir), **DATA)
    res = ResidentLatentDataModule(data_path=str(data_dir), **DATA, device=dev, resident_val=True, val_batches=VB, val_frame_budget=1024)
    assert [f.parent.name for f in host.val_set._files()] == ["0000", "0001", "0002", "0003"]
    out = {}
    for limit in (None, 3):
        shell = Trainer(precision="32", default_root_dir=str(tmp_path), limit_val_batches=limit)
        for name, dm in (("host", host), ("resident", res)):
            seen = []
            tr.validation_step = pinned(tr, dm, seen, dev)
            Counted.reads.clear()
            vals = shell.validate(tr, dm, dev)
            out[name, limit] = (vals, sorted(seen), list(Counted.reads))
            assert sorted(vals) == sorted(f"val/{k}" for k in VAL_LOG_NAMES)
        (a, maps_a, reads_a), (b, maps_b, reads_b) = out["resident", limit], out["host", limit]
        assert maps_a == maps_b == list(range(4 if limit is None else 3)), "the two paths validated different maps"
        groups = len(res.val_feed.groups)
        assert groups == 2 and len(res.val_feed.short) == 0
        assert reads_a == ["cpu"] * groups, f"host reads of a grouped validation: {reads_a}"
        assert len(reads_b) == 4 * len(maps_b)                   # the per-map path: four float() a map
        for k in a:
            rel = abs(a[k] - b[k]) / abs(b[k])
            print(f"{mode} limit {limit} {k}: resident {a[k]:.8g}, host {b[k]:.8g}, relative {rel:.2e}")
            assert rel <= BOUND[mode], (mode, limit, k, a[k], b[k])
    assert out["resident", None][0] != out["resident", 3][0]


def test_off_by_default(dev, data_dir):
    dm = ResidentLatentDataModule(data_path=str(data_dir), **DATA, device=dev)
    assert isinstance(dm.val_dataloader(), DataLoader) and dm.val_feed is None and not dm.resident_val
    batch = next(iter(dm.val_dataloader()))
    assert len(batch) == 4 and batch[1].shape == (1, D.emb_dim, FRAMES[0])


def test_refusals(dev, data_dir, tmp_path):
    shell = Trainer(precision="32", default_root_dir=str(tmp_path))
    data = dict(DATA, data_path=str(data_dir))
    with pytest.raises(ValueError, match="data.resident_val.*data.resident: true"):
        build_latent_data(dict(data, resident_val=True), shell, val_batches=VB)
    with pytest.raises(ValueError, match="data.resident_val.*data.resident: true"):
        build_latent_data(dict(data, val_frame_budget=1024), shell, val_batches=VB)
    with pytest.raises(ValueError, match="data.val_frame_budget.*data.resident_val: true"):
        build_latent_data(dict(data, resident=True, resident_val=False, val_frame_budget=1024), shell, val_batches=VB)
    with pytest.raises(ValueError, match="data.resident_val.*style-only"):
        build_latent_data(dict(data, resident=True, resident_val=True), shell, style_only=True, val_batches=VB)
    # both stores under one resident_max_gb
    dm = build_latent_data(dict(data, resident=True, resident_val=True), shell, val_batches=VB)
    assert type(dm) is ResidentLatentDataModule and dm.val_feed is None                  # built on first use
    feed = dm.val_dataloader()
    assert dm.val_dataloader() is feed and len(feed.store) == 4 and feed.frame_budget == 131072 and feed.val_batches == VB
    train_bytes, val_bytes = dm.store.nbytes, feed.store.nbytes
    fits = build_latent_data(dict(data, resident=True, resident_val=True, resident_max_gb=(train_bytes + val_bytes) / 2 ** 30), shell, val_batches=VB)
    assert len(fits.val_dataloader().store) == 4
    assert train_bytes < train_bytes + val_bytes - 1
    tight = build_latent_data(dict(data, resident=True, resident_val=True, resident_max_gb=(train_bytes + val_bytes - 1) / 2 ** 30), shell,
                              val_batches=VB)
    made, empty = [], torch.empty

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


# ================================================================================================================ fit-denoiser
def test_fit_denoiser_resident_val(dev, tmp_path, monkeypatch):
    cfg = _ragged_cfg(tmp_path, dev)                             # eight maps, the first two (70 and 150 frames) held out; val_batches 8
    cfg["trainer"].update(max_steps=4, val_check_interval=3, limit_val_batches=None)
    counts, groups = {}, {}
    step = DiffusionTrainer.validation_step

    def counting(self, batch, batch_idx, *a, **k):
        logs = step(self, batch, batch_idx, *a, **k)
        counts[run] = counts.get(run, 0) + (logs["loss"].numel())
        groups[run] = groups.get(run, 0) + isinstance(batch, RaggedLatentValBatch)
        return logs
    monkeypatch.setattr(DiffusionTrainer, "validation_step", counting)
    val = {}
    for run, on in (("on", True), ("off", False)):
        c = copy.deepcopy(cfg)
        c["data"].update(resident=True, resident_val=on, resident_max_gb=0.5)
        c["trainer"]["default_root_dir"] = str(tmp_path / run)
        path = tmp_path / f"{run}.yml"
        path.write_text(yaml.safe_dump(c))
        module, trainer = fit_denoiser(str(path))
        assert trainer.global_step == 4
        lines = [json.loads(l) for l in open(tmp_path / run / "metrics.jsonl")]
        val[run] = [l for l in lines if "val/loss" in l]
        assert len(val[run]) == 1 and all(np.isfinite(val[run][0][f"val/{k}"]) for k in VAL_LOG_NAMES)
        ck = torch.load(tmp_path / run / "checkpoints" / "best.ckpt", map_location="cpu", weights_only=False)
        assert ck["global_step"] == 3 and ck["best_val"] == val[run][0]["val/loss"]
    assert counts == {"on": 2, "off": 2} and groups == {"on": 1, "off": 0}
    assert sorted(val["on"][0]) == sorted(val["off"][0])
