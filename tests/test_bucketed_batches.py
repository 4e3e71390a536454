"""Frame-budget, length-bucketed ragged batches: LatentDataModule(seq_len=None, batch_frames=F), the engine switching between their
(B, Lpad) plans, and `fit-denoiser` on them.

  1. the loader: every batch within the frame budget and the song cap, padded to its own longest map, zero padding, every training map
     exactly once per epoch, reproducible from the seed, and less padding than fixed-count collation of the same maps;
  2. the configurations it refuses;
  3. plan switches X -> Y -> X under OD_DETERMINISTIC: the second X step is the first, bit for bit, Y is what a fresh model computes on Y
     alone, with the padding NaN-poisoned throughout;
  4. `fit-denoiser` with data.batch_frames from the YAML alone.
The kernel-running tests run on the emulator and on the MI355X (the `dev` fixture).
"""
import json

import numpy as np
import pytest
import torch
import yaml

from oracle import denoiser_oracle as O
from osu_dreamer_amd import det
from osu_dreamer_amd.data import LatentDataModule, RaggedLatentBatch, cut_batches, write_synthetic_dataset
from osu_dreamer_amd.engine import DenoiserEngine
from osu_dreamer_amd.fit import fit_denoiser
from kernel_backend import dev  # noqa: F401
from test_model_parity import make_trainer
from test_ragged_train import NAN, _dims, _ragged_cfg, step

# 48 maps of 20 .. 600 frames in a scrambled order (i * 37 mod 59 walks 0 .. 58 without repeating for i < 59); 4 are held out
FRAMES = [20 + (i * 37 % 59) * 10 for i in range(48)]
PAD, BUDGET, CAP, POOL, MAX_LEN = 64, 1280, 16, 16, 600


def _roundup(n):
    return (n + PAD - 1) // PAD * PAD


@pytest.fixture(scope="module")
def dataset(tmp_path_factory):
    root = tmp_path_factory.mktemp("bucketed")
    write_synthetic_dataset(str(root), n_maps=len(FRAMES), frames=FRAMES, a_dim=16, emb_dim=6, style_dim=8, seed=11)
    styles = {}
    for i, n in enumerate(FRAMES):
        with np.load(root / f"{i:04d}" / "0.latent.npz") as f:
            styles[i] = torch.from_numpy(f["s"])
    return root, styles


def _module(root, **kw):
    args = dict(batch_size=CAP, seq_len=None, num_workers=0, max_val_count=4, max_val_frac=.3, data_path=str(root), max_len=MAX_LEN,
                pad_multiple=PAD, batch_frames=BUDGET, bucket_pool=POOL)
    args.update(kw)
    return LatentDataModule(**args)


def _epoch(dm, seed=0):
    torch.manual_seed(seed)
    return list(dm.train_dataloader())


def _efficiency(batches):
    return sum(int(b.lengths.sum()) for b in batches) / sum(b.z.shape[0] * b.z.shape[-1] for b in batches)


# ---------------------------------------------------------------- 1. the loader
def test_bucketed_loader_properties(dataset):
    """44 training maps of 20 .. 600 frames, batch_frames 1280, cap 16, pools of 16.  Padding efficiency sum(lengths) / sum(B * Lpad) of the
    epoch, worked out on the CPU while this test was written: 0.826 bucketed (17 batches) against 0.555 for batch_size 4 fixed-count
    collation of the same maps (11 batches; the existing loader, no batch_frames) — the inequality holds with a margin of 0.27."""
    root, styles = dataset
    dm = _module(root)
    batches = _epoch(dm)
    seen = []
    for bt in batches:
        assert isinstance(bt, RaggedLatentBatch)
        h, z, s, labels, lengths = bt
        B, Lpad = z.shape[0], z.shape[-1]
        assert 1 <= B <= CAP and B * Lpad <= BUDGET, (B, Lpad)
        assert Lpad == _roundup(int(lengths.max())) and lengths.dtype == torch.int64 and lengths.shape == (B,)
        assert h.shape == (B, 16, Lpad) and s.shape == (B, 8) and labels.shape == (B, 5)
        for b in range(B):
            n = int(lengths[b])
            assert torch.count_nonzero(h[b, :, n:]).item() == 0 and torch.count_nonzero(z[b, :, n:]).item() == 0
            assert torch.count_nonzero(z[b, :, :n]).item() > 0
            i = next(i for i, sv in styles.items() if torch.equal(sv, s[b]))
            assert n == min(FRAMES[i], MAX_LEN)
            seen.append(i)
    # hold_out_mapsets keeps the first four mapsets for validation: the other 44 appear exactly once each
    assert sorted(seen) == list(range(4, len(FRAMES)))
    assert len({(b.z.shape[0], b.z.shape[-1]) for b in batches}) > 1
    # the same seed gives the same sequence of batches; another seed shuffles the pools' batches differently
    again = _epoch(_module(root))
    assert len(again) == len(batches)
    for a, b in zip(batches, again):
        assert all(torch.equal(x, y) for x, y in zip(a, b))
    other = _epoch(_module(root), seed=1)
    assert any(a.z.shape != b.z.shape or not torch.equal(a.s, b.s) for a, b in zip(batches, other))
    # less padding than fixed-count batches of the same maps
    fixed = _epoch(LatentDataModule(batch_size=4, seq_len=None, num_workers=0, max_val_count=4, max_val_frac=.3, data_path=str(root),
                                    max_len=MAX_LEN, pad_multiple=PAD))
    assert sum(b.z.shape[0] for b in fixed) == 44                       # (44 = 11 x 4: drop_last drops nothing)
    eff, eff_fixed = _efficiency(batches), _efficiency(fixed)
    print(f"MEASURED padding efficiency: bucketed {eff:.3f} in {len(batches)} batches, fixed-count {eff_fixed:.3f} in {len(fixed)} batches")
    assert eff > eff_fixed, (eff, eff_fixed)


def test_one_song_batches_and_the_partial_pool(dataset):
    """A cap of one song: every batch is one song and still a RaggedLatentBatch; a pool larger than the stream is cut at its end."""
    root, _ = dataset
    batches = _epoch(_module(root, batch_size=1, bucket_pool=1000))
    assert len(batches) == 44 and all(isinstance(b, RaggedLatentBatch) and b.z.shape[0] == 1 for b in batches)
    assert cut_batches([64, 1, 64, 200, 65], 256, 16, 64) == [[3], [4, 0], [2, 1]]      # ties keep arrival order; 65 opens an Lpad of 128
    assert cut_batches([10, 10, 10], 1 << 20, 2, 64) == [[0, 1], [2]]                   # the cap on songs


# ---------------------------------------------------------------- 2. refusals
@pytest.mark.parametrize("kw,match", [
    (dict(seq_len=32, max_len=None), "seq_len"),
    (dict(max_len=None), "max_len"),
    (dict(max_len=1300), "batch_frames"),            # roundup(1300, 64) = 1344 > 1280
    (dict(bucket_pool=0), "bucket_pool"),
    (dict(batch_size=0), "batch_size"),
    (dict(batch_frames=None), "bucket_pool"),        # a pool without a frame budget
])
def test_bucketed_loader_refusals(dataset, kw, match):
    with pytest.raises(ValueError, match=match):
        _module(dataset[0], **kw)


# ---------------------------------------------------------------- 3. plan switches
X_LENS, X_LPAD = [130, 65, 1], 192
Y_LENS, Y_LPAD = [64, 40, 33, 17, 1], 64


def _poisoned(d, lens, Lpad, seed):
    data = O.synthetic_batch(d, len(lens), Lpad, seed=seed)
    for b, n in enumerate(lens):
        for k in ("h", "z", "x0"):
            data[k][b, :, n:] = NAN
    return data


@pytest.mark.parametrize("dt", [None, torch.bfloat16], ids=["fp32", "bf16"])
def test_plan_switches_keep_every_plan_clean(dev, dt):
    """X (B = 3, Lpad = 192) -> Y (B = 5, Lpad = 64) -> X on one model, gradients zeroed in between, no optimizer step, OD_DETERMINISTIC: the
    second X step's loss terms and gradient arena are the first's bit for bit, Y's are those of a freshly built model stepping on Y alone,
    and the engine came back to X's workspace instead of building a third."""
    d = _dims(32, 2, 2, 2)
    P = O.init_params(d, seed=101)
    for k in P:
        if any(z in k for z in ("ssg1.", "ssg2.", "proj_out.", "u_mod.")):
            P[k] = torch.randn(P[k].shape, generator=torch.Generator().manual_seed(len(k))) * 0.05
    X, Y = _poisoned(d, X_LENS, X_LPAD, 102), _poisoned(d, Y_LENS, Y_LPAD, 103)
    try:
        det.force(True)
        tr = make_trainer(d, P, dev)
        tr.diffusion.compute_dtype = dt
        runs = []
        for data, lens in ((X, X_LENS), (Y, Y_LENS), (X, X_LENS)):
            loss, logs, _, _ = step(tr, data, dev, lengths=lens)
            runs.append((loss, logs, tr.diffusion.arena.grad.detach().cpu().clone()))
        eng = tr.diffusion.engine
        fresh = make_trainer(d, P, dev)
        fresh.diffusion.compute_dtype = dt
        loss, logs, _, _ = step(fresh, Y, dev, lengths=Y_LENS)
        alone = (loss, logs, fresh.diffusion.arena.grad.detach().cpu().clone())
    finally:
        det.force(None)
    for what, a, b in (("the second X step against the first", runs[2], runs[0]), ("Y between the X steps against Y alone", runs[1], alone)):
        assert np.isfinite(a[0]) and not bool(torch.isnan(a[2]).any()), what
        assert a[0] == b[0] and a[1] == b[1], (what, a[:2], b[:2])
        assert torch.equal(a[2].view(torch.int32), b[2].view(torch.int32)), f"{what}: the gradient arena differs"
    assert float(runs[0][2].abs().max()) > 0 and not torch.equal(runs[0][2], runs[1][2])
    assert (eng.plan_switches, eng.plan_builds) == (3, 2), "the engine must return to X's cached workspace"


# ---------------------------------------------------------------- 4. the command
STEPS = 8


def test_fit_denoiser_with_batch_frames(dev, tmp_path, monkeypatch):
    """`fit-denoiser` from a YAML with data.batch_frames on the tiny config: six training maps of (96, 128, 33, 128, 90, 61) frames after
    max_len, a budget of 256 frames -> an epoch of three batches, (2, 128) twice and (2, 64).  Eight optimizer steps, one metrics record
    each, every loss finite, and the engine planned more than one (B, Lpad)."""
    cfg = _ragged_cfg(tmp_path, dev)
    cfg["data"].update(batch_size=4, batch_frames=256, bucket_pool=6)
    path = tmp_path / "bucketed.yml"
    path.write_text(yaml.safe_dump(cfg))
    planned, plan = set(), DenoiserEngine.plan

    def recording_plan(self, B, L, Ba, dtype, train, x3=False, lens=None, offs=None):
        if train and lens is not None:
            planned.add((B, L))
        return plan(self, B, L, Ba, dtype, train, x3=x3, lens=lens, offs=offs)

    monkeypatch.setattr(DenoiserEngine, "plan", recording_plan)
    module, trainer = fit_denoiser(str(path))
    assert trainer.global_step == STEPS and int(module.diffusion_ema.n_averaged) == STEPS
    lines = [json.loads(l) for l in open(tmp_path / "run" / "metrics.jsonl")]
    train = [l for l in lines if "train/loss" in l]
    assert [l["step"] for l in train] == list(range(1, STEPS + 1))
    assert all(np.isfinite(l[k]) for l in train for k in ("train/loss", "train/osl", "train/del", "train/u_mape"))
    assert len([l for l in lines if "val/loss" in l]) == 1
    print(f"MEASURED planned (B, Lpad): {sorted(planned)}")
    assert planned == {(2, 128), (2, 64)}
