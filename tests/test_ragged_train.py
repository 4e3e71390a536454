"""Ragged training of the denoiser: DiffusionTrainer.forward(..., lengths=), its backward, the loader and the command.

The ragged step is defined by the dense one: on a padded (B, Lpad) batch whose row b is valid for lengths[b] frames, the loss is the mean
over b of the dense step on sequence b alone at L = lengths[b] (same t[b], x0[b]), and so is every parameter gradient.  The dense step is
pinned against the reference by tests/golden (test_model_parity.py), so:
  1. with lengths = [L] * B the ragged step meets the dense fixtures' own tolerances against the reference's values;
  2. a ragged batch (lengths 130, 65, 64, 1 in Lpad = 192) equals the mean of its four dense single-song steps, per parameter tensor, within
     4 x the distance the EXISTING code shows between a dense step on one song alone and that song's share of a dense equal-length batch
     (and at least 8 eps of the compute dtype, relative to the gradient's norm);
  3. the padding is never read: zero padding against NaN padding (x0, x1 and h — the trainer zero-fills h), bit for bit under OD_DETERMINISTIC:
     loss, gradient arena, weights and EMA after one optimizer step;
  4. a ragged plan never takes the fused attention backward (GPU, Lpad = 2112, OD_ATTN_BWD_FUSED=1);
  5. LatentDataModule(seq_len=None, batch_size=3) collates whole maps; fit_denoiser trains on them; two devices are refused;
  6. forward(..., lengths=) under no_grad is what it was: each song alone, and untouched by a ragged training step in between.
Runs on the emulator and on the MI355X (the `dev` fixture), like test_model_parity.py's step tests.
"""
import json
import os

import numpy as np
import pytest
import torch
import yaml

from oracle import denoiser_oracle as O
from osu_dreamer_amd import det
from osu_dreamer_amd.data import LatentDataModule, RaggedLatentBatch, write_synthetic_dataset
from osu_dreamer_amd.fit import DEFAULT_CONFIG, fit_denoiser
from kernel_backend import dev, rel_l2  # noqa: F401
from test_model_parity import BF16_FLOOR, BF16_K, dims_of, inputs, load, make_trainer

NAN = float("nan")
EPS = {None: float(torch.finfo(torch.float32).eps), torch.bfloat16: float(torch.finfo(torch.bfloat16).eps)}


def step(tr, data, dev, lengths=None, rows=None, L=None, backward=True):
    """One pinned training step of `tr` on rows `rows` (default all) cut to L frames (default all): loss, logs and a copy of every gradient."""
    model = tr.diffusion
    sl = slice(None) if rows is None else rows
    cut = lambda x: x[sl][..., :L].contiguous().to(dev) if x.dim() == 3 else x[sl].contiguous().to(dev)   # noqa: E731
    opt = tr.configure_optimizers()["optimizer"]
    opt.zero_grad()
    loss, logs = tr(model, cut(data["h"]), cut(data["z"]), cut(data["s"]), None, lengths=lengths, t=cut(data["t"]), x0=cut(data["x0"]))
    if backward:
        loss.backward()
    grads = {k: p.grad.detach().cpu().clone() for k, p in model.named_parameters()} if backward else None
    return float(loss.detach()), {k: float(v) for k, v in logs.items()}, grads, opt


# ---------------------------------------------------------------- 1. the reference anchor
@pytest.mark.parametrize("name", ["tiny_b3_l40", "tiny_hd128_b2_l130"])
def test_full_lengths_meet_the_dense_fixture_fp32(dev, name):
    """lengths = [L] * B on a dense fp32 fixture of the reference: test_model_parity.run_case's tolerances for the loss terms and every gradient."""
    fx = load(name)
    d = dims_of(fx)
    P, data = inputs(fx, d)
    tr = make_trainer(d, P, dev)
    data = dict(data, t=fx["t_used"])
    B, L = data["z"].shape[0], data["z"].shape[-1]
    loss, logs, grads, _ = step(tr, data, dev, lengths=[L] * B)
    assert tr.diffusion.engine.varlen
    assert loss == pytest.approx(float(fx["loss"]), rel=5e-5)
    for k in ("osl", "del", "u_mape"):
        assert logs[k] == pytest.approx(float(fx["log_" + k]), rel=1e-4)
    assert float(tr.diffusion.arena.grad.double().norm()) == pytest.approx(float(fx["grad_norm"]), rel=2e-4)
    for k, g in grads.items():
        if "grad." + k in fx:
            assert rel_l2(g, fx["grad." + k]) < 1e-3, k
        else:                                        # a fixture that stores a strided sub-sample and the norm of each gradient
            n = g.numel()
            assert float(g.norm()) == pytest.approx(float(fx["gradnorm." + k]), rel=3e-3, abs=1e-6), k
            assert torch.allclose(g.flatten()[::max(1, n // 64)][:64], fx["gradsub." + k], rtol=2e-2, atol=2e-5 * float(fx["gradnorm." + k]) + 1e-7), k


@pytest.mark.parametrize("name", ["train_bf16_tiny_b3_l40", "train_bf16_tiny_hd128_b2_l130"])
def test_full_lengths_meet_the_dense_fixture_bf16(dev, name):
    """The same in bf16 compute, held as test_model_parity.run_bf16_training_case holds the dense step: within BF16_K x the reference's own
    bf16-autocast error per tensor."""
    fx = load(name)
    d = dims_of(fx)
    seed = int(fx["seed"])
    P = O.init_params(d, seed=seed)
    data = dict(O.synthetic_batch(d, int(fx["B"]), int(fx["L"]), seed=seed + 1), t=fx["t_used"])
    tr = make_trainer(d, P, dev)
    tr.diffusion.compute_dtype = torch.bfloat16
    loss, _, grads, _ = step(tr, data, dev, lengths=[int(fx["L"])] * int(fx["B"]))
    assert tr.diffusion.engine.varlen
    ref32, ref16 = float(fx["f32.loss"]), float(fx["bf16.loss"])
    assert abs(loss - ref32) <= BF16_K * abs(ref16 - ref32) + 2e-3 * ref32, (loss, ref32, ref16)
    gn, gn32, gn16 = float(tr.diffusion.arena.grad.double().norm()), float(fx["f32.grad_norm"]), float(fx["bf16.grad_norm"])
    assert abs(gn - gn32) <= BF16_K * abs(gn16 - gn32) + 5e-3 * gn32, (gn, gn32, gn16)
    for k, g in grads.items():
        if "f32.grad." + k in fx:
            r32, r16, mine = fx["f32.grad." + k], fx["bf16.grad." + k], g
        else:
            r32, r16, n = fx["f32.gradsub." + k], fx["bf16.gradsub." + k], g.numel()
            mine, n32 = g.flatten()[::max(1, n // 64)][:64], float(fx["f32.gradnorm." + k])
            assert abs(float(g.norm()) - n32) <= BF16_K * abs(float(fx["bf16.gradnorm." + k]) - n32) + 2e-2 * n32 + 1e-7, k
        if float(r32.norm()) == 0:
            continue
        assert rel_l2(mine, r32) <= BF16_K * rel_l2(r16, r32) + BF16_FLOOR, k


# ---------------------------------------------------------------- 2. ragged against per-song dense
LENS, LPAD = [130, 65, 64, 1], 192
# (head_dim, radius, heads, blocks): every head dim the kernel pair has and both conv radii of the issue (k = 3 and k = 5) on the smallest
# network that has every kind of layer (the emulator's attention at head_dim 128 sets the test's time), and two heads in two blocks — the
# per-head offsets of the varlen backward and d.qkv reused from block to block — at head_dim 32
RAGGED_CONFIGS = [(32, 1, 1, 1), (64, 2, 1, 1), (128, 1, 1, 1), (32, 2, 2, 2)]


def _dims(hd, radius, heads=1, depth=1):
    return O.Dims(global_cond_dim=32, backbone_dim=64, n_heads=heads, head_dim=hd, depth=depth, expand=2, radius=radius, u_head_dim=8)


def _mean_of_single_steps(d, P, data, dev, dt, lens):
    """(1 / B) sum_b of the dense step on song b alone at L = lens[b]."""
    B = len(lens)
    loss, logs, grads = 0.0, {}, None
    for b, Lb in enumerate(lens):
        tr = make_trainer(d, P, dev)
        tr.diffusion.compute_dtype = dt
        l, lg, g, _ = step(tr, data, dev, rows=slice(b, b + 1), L=Lb)
        assert not tr.diffusion.engine.varlen
        loss += l / B
        for k, v in lg.items():
            logs[k] = logs.get(k, 0.0) + v / B
        grads = {k: v.double() / B for k, v in g.items()} if grads is None else {k: grads[k] + v.double() / B for k, v in g.items()}
    return loss, logs, grads


@pytest.mark.parametrize("dt", [None, torch.bfloat16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("hd,radius,heads,depth", RAGGED_CONFIGS, ids=[f"hd{h}-r{r}-{n}x{k}" for h, r, n, k in RAGGED_CONFIGS])
def test_ragged_step_is_the_mean_of_the_single_song_steps(dev, hd, radius, heads, depth, dt):
    """One ragged training_step + backward on B = 4, lengths (130, 65, 64, 1), Lpad = 192 against the mean of the four dense single-song
    steps, per parameter tensor, relative to the gradient's norm.  The yardstick is measured here with the existing dense code alone: the
    distance between the mean of two single-song dense steps and ONE dense step on the same two songs as an equal-length batch (L = 65) —
    in fp32 the summation order of the weight-gradient sums; in bf16 also the stored activations' rounding meeting another batch factor.
    Bound: 4 x that, and at least 8 eps of the compute dtype.
    Measured, worst tensor of each case (emulator | MI355X): fp32 ragged 1.0e-7 .. 1.7e-7 | 1.0e-7 .. 1.7e-7 against a yardstick of
    1.6e-7 .. 2.0e-7 | 1.6e-7 .. 1.9e-7 (bound 9.5e-7 = 8 eps); bf16 ragged 1.0e-7 .. 2.5e-7 | 1.0e-7 .. 1.7e-7, yardstick 0.9e-7 .. 1.1e-7 |
    0.7e-7 .. 1.0e-7 (bound 6.2e-2 = 8 eps of bf16): at this width every row of a sequence goes through the same roundings in both
    runs, and the batch mean's 1 / 4 is exact in bf16.  (A wider two-head, two-block model — another GEMM tile choice per row count —
    measured 1.5e-3 .. 5.3e-3 in bf16 against a yardstick of 3.4e-3 .. 4.7e-3.)  Loss terms: within 2e-7 relative in fp32, 4e-6 in bf16."""
    d = _dims(hd, radius, heads, depth)
    P = O.init_params(d, seed=50 + hd + radius)
    for k in P:                                   # (the reference zero-initialises these: un-zero them so every gradient is live)
        if any(z in k for z in ("ssg1.", "ssg2.", "proj_out.", "u_mod.")):
            P[k] = torch.randn(P[k].shape, generator=torch.Generator().manual_seed(len(k))) * 0.05
    data = O.synthetic_batch(d, len(LENS), LPAD, seed=60 + hd)
    # the yardstick: existing code only
    L0 = 65
    tr = make_trainer(d, P, dev)
    tr.diffusion.compute_dtype = dt
    two = {k: v[1:3] for k, v in data.items()}
    _, _, gb, _ = step(tr, two, dev, L=L0)
    _, _, gs = _mean_of_single_steps(d, P, two, dev, dt, [L0, L0])
    margin = {k: float((gb[k].double() - gs[k]).norm() / (gs[k].norm() + 1e-300)) for k in gb}
    # the ragged step, through training_step
    tr = make_trainer(d, P, dev)
    tr.diffusion.compute_dtype = dt
    opt = tr.configure_optimizers()["optimizer"]
    opt.zero_grad()
    batch = RaggedLatentBatch(data["h"].to(dev), data["z"].to(dev), data["s"].to(dev), torch.zeros(len(LENS), 5, device=dev), torch.tensor(LENS))
    h, z, s, labels, lengths = batch
    loss, logs = tr(tr.diffusion, h, z, s, labels, lengths=lengths, t=data["t"].to(dev), x0=data["x0"].to(dev))
    loss.backward()
    assert tr.diffusion.engine.varlen and not tr.diffusion.engine.fused_attn_bwd()
    rl, rlogs, rg = _mean_of_single_steps(d, P, data, dev, dt, LENS)
    assert float(loss.detach()) == pytest.approx(rl, rel=1e-5 if dt is None else 1e-4)
    for k in ("osl", "del", "u_mape"):
        assert float(logs[k]) == pytest.approx(rlogs[k], rel=1e-5 if dt is None else 1e-4), k
    worst, worst_m = 0.0, 0.0
    for k, p in tr.diffusion.named_parameters():
        e = float((p.grad.detach().cpu().double() - rg[k]).norm() / (rg[k].norm() + 1e-300))
        bound = max(4 * margin[k], 8 * EPS[dt])
        worst, worst_m = max(worst, e), max(worst_m, margin[k])
        assert e <= bound, f"{k}: ragged step {e:.3e} from the mean of the single-song steps, bound {bound:.3e} (yardstick {margin[k]:.3e})"
    print(f"MEASURED ragged hd{hd} r{radius} {heads} heads x {depth} blocks {'fp32' if dt is None else 'bf16'}: worst tensor {worst:.3e}, worst yardstick {worst_m:.3e}, "
          f"loss {float(loss.detach()):.6f} against {rl:.6f}")


# ---------------------------------------------------------------- 3. padding is never read
@pytest.mark.parametrize("dt", [None, torch.bfloat16], ids=["fp32", "bf16"])
def test_padding_is_never_read(dev, dt):
    d = _dims(64, 2)
    P = O.init_params(d, seed=71)
    for k in P:
        if any(z in k for z in ("ssg1.", "ssg2.", "proj_out.", "u_mod.")):
            P[k] = torch.randn(P[k].shape, generator=torch.Generator().manual_seed(len(k))) * 0.05
    data = O.synthetic_batch(d, len(LENS), LPAD, seed=72)
    out = {}
    try:
        det.force(True)
        for fill in (0.0, NAN):
            dd = {k: v.clone() for k, v in data.items()}
            for b, Lb in enumerate(LENS):
                for k in ("h", "z", "x0"):              # the trainer zero-fills h's padding itself: NaN there must not reach a GEMM
                    dd[k][b, :, Lb:] = fill
            tr = make_trainer(d, P, dev)
            tr.diffusion.compute_dtype = dt
            loss, _, _, opt = step(tr, dd, dev, lengths=LENS)
            opt.max_grad_norm = 1.0
            g = tr.diffusion.arena.grad.detach().cpu().clone()
            opt.step()
            tr.on_train_batch_end()
            out[fill == 0.0] = (loss, g, tr.diffusion.arena.data.detach().cpu().clone(), tr.diffusion_ema.module.arena.data.detach().cpu().clone())
    finally:
        det.force(None)
    a, b = out[True], out[False]
    assert not bool(torch.isnan(b[1]).any()) and a[0] == b[0]
    for x, y, what in zip(a[1:], b[1:], ("gradient arena", "weights", "EMA")):
        assert torch.equal(x.view(torch.int32), y.view(torch.int32)), f"{what} differs between zero and NaN padding"
    assert not torch.equal(a[2], P_arena(tr, P)), "the optimizer step must have moved the weights"


def P_arena(tr, P):
    m = type(tr.diffusion)(tr.diffusion.emb_dim, tr.diffusion.a_dim, tr.diffusion.style_dim, tr.diffusion.args)
    m.load_state_dict(P)
    return m.arena.data.detach().cpu()


# ---------------------------------------------------------------- 4. kernel choice
@pytest.mark.gpu
def test_ragged_step_never_takes_the_fused_attention_backward(monkeypatch):
    if not torch.cuda.is_available():
        pytest.skip("no GPU is visible")
    from osu_dreamer_amd import _lib
    _lib._lib = None
    _lib.lib()
    dev = torch.device("cuda:0")
    monkeypatch.setenv("OD_ATTN_BWD_FUSED", "1")
    d = O.Dims(global_cond_dim=64, backbone_dim=128, n_heads=2, head_dim=64, depth=2, expand=2, radius=2, u_head_dim=16)
    P = O.init_params(d, seed=81)
    Lpad, lens = 2112, [2112, 1500, 65]
    data = O.synthetic_batch(d, len(lens), Lpad, seed=82)
    tr = make_trainer(d, P, dev)
    tr.diffusion.compute_dtype = torch.bfloat16
    loss, _, grads, _ = step(tr, data, dev, lengths=lens)
    eng = tr.diffusion.engine
    assert eng.varlen and not eng.fused_attn_bwd() and eng.attn_bwd_passes() == 7 and eng.attn_status_ptr() == 0
    assert np.isfinite(loss) and all(bool(torch.isfinite(g).all()) for g in grads.values())
    # the same plan shape without lengths does take it (the switch is honoured where a fused form exists)
    tr2 = make_trainer(d, P, dev)
    tr2.diffusion.compute_dtype = torch.bfloat16
    step(tr2, data, dev)
    assert tr2.diffusion.engine.fused_attn_bwd() and tr2.diffusion.engine.attn_status_ptr() != 0


# ---------------------------------------------------------------- 5. loader and command
def test_ragged_loader(tmp_path):
    frames = [70, 150, 96, 200, 33, 128, 90, 61]
    write_synthetic_dataset(str(tmp_path), n_maps=len(frames), frames=frames, a_dim=16, emb_dim=6, style_dim=8, seed=3)
    maps = {}
    for i, n in enumerate(frames):
        with np.load(tmp_path / f"{i:04d}" / "0.latent.npz") as f:
            maps[i] = (torch.from_numpy(f["z"]), torch.from_numpy(np.load(tmp_path / f"{i:04d}" / "h.npy")), torch.from_numpy(f["s"]))
    torch.manual_seed(0)
    dm = LatentDataModule(batch_size=3, seq_len=None, num_workers=0, max_val_count=2, max_val_frac=.3, data_path=str(tmp_path),
                          max_len=100, pad_multiple=64)
    batches = list(dm.train_dataloader())
    assert len(batches) == 2                                     # 6 training maps, drop_last
    windows = 0
    for bt in batches:
        assert isinstance(bt, RaggedLatentBatch)
        h, z, s, labels, lengths = bt
        N, Lpad = 3, z.shape[-1]
        assert h.shape == (N, 16, Lpad) and z.shape == (N, 6, Lpad) and s.shape == (N, 8) and labels.shape == (N, 5) and lengths.shape == (N,)
        assert Lpad % 64 == 0 and Lpad - 64 < int(lengths.max()) <= Lpad and int(lengths.max()) <= 100
        for b in range(N):
            n = int(lengths[b])
            assert torch.count_nonzero(h[b, :, n:]).item() == 0 and torch.count_nonzero(z[b, :, n:]).item() == 0
            i = next(i for i, m in maps.items() if torch.equal(m[2], s[b]))
            zf, hf, _ = maps[i]
            assert n == min(frames[i], 100)
            # the window is a contiguous piece of its map, the same piece of h and z
            starts = [o for o in range(frames[i] - n + 1) if torch.equal(zf[:, o:o + n], z[b, :, :n])]
            assert len(starts) == 1 and torch.equal(hf[:, starts[0]:starts[0] + n], h[b, :, :n])
            windows += frames[i] > 100
    assert windows >= 1
    # with an integer seq_len nothing changes: the default collate's 4-tuple of fixed windows
    dm2 = LatentDataModule(batch_size=2, seq_len=32, num_workers=0, max_val_count=2, max_val_frac=.3, data_path=str(tmp_path))
    b2 = next(iter(dm2.train_dataloader()))
    assert len(b2) == 4 and b2[1].shape == (2, 6, 32)
    with pytest.raises(ValueError):
        LatentDataModule(batch_size=2, seq_len=32, num_workers=0, data_path=str(tmp_path), max_len=64)


def _ragged_cfg(tmp_path, dev):
    cfg = yaml.safe_load(open(DEFAULT_CONFIG))
    cfg["model"].update(emb_dim=6, a_dim=16, style_dim=8)
    cfg["model"]["diffusion_args"] = dict(global_cond_dim=32, u_head_dim=8, backbone_dim=64,
                                          backbone_args=dict(head_dim=32, n_heads=2, depth=1, expand=2, radius=2))
    frames = [70, 150, 96, 200, 33, 128, 90, 61]
    write_synthetic_dataset(str(tmp_path / "data"), n_maps=len(frames), frames=frames, a_dim=16, emb_dim=6, style_dim=8, seed=1)
    cfg["data"].update(data_path=str(tmp_path / "data"), seq_len=None, batch_size=3, num_workers=0, shuffle_buffer_size=1, max_val_count=2,
                       max_per_map=-1, max_len=128, pad_multiple=64)
    cfg["trainer"].update(max_steps=8, log_every_n_steps=1, val_check_interval=8, limit_val_batches=1,
                          default_root_dir=str(tmp_path / "run"), precision="32" if dev.type == "cpu" else "bf16-mixed")
    cfg["seed_everything"] = 7
    return cfg


STEPS = 8


def test_fit_denoiser_ragged(dev, tmp_path, monkeypatch):
    """`fit-denoiser` with `data.seq_len: null` on the tiny config, as test_fit.py drives the fixed-window run: eight ragged steps, every loss
    finite, one validation, the EMA count, the checkpoint's layout, reload and resume — and the loss decreasing.  The logged losses cannot
    show that: each step draws its own t, and with the weights frozen they already move between 24 and 35 from step to step.  So the decrease is
    measured on pinned draws: one ragged batch of three training maps with fixed t and x0, evaluated with the weights the run started from
    and with the weights it ended with.  As in test_fit.py the reference's zero-initialised tensors are un-zeroed first (here through the
    command's own model builder), so that from the first step the gradient runs through the whole backbone, the varlen attention and conv
    backward included.  Measured (emulator, fp32, 8 steps at lr 1e-3): 35.07 -> 28.78; asserted: below 0.95 x the start."""
    from osu_dreamer_amd import fit as fit_mod
    from osu_dreamer_amd.data import collate_ragged, load_latents
    cfg = _ragged_cfg(tmp_path, dev)
    cfg["model"]["opt_args"] = dict(lr=1e-3, weight_decay=0.0)
    cfg["model"]["schedule_args"] = dict(warmup_steps=1, warmup_init=1.0, decay_start=30000)
    path = tmp_path / "ragged.yml"
    path.write_text(yaml.safe_dump(cfg))
    build, start = fit_mod.build_from_config, {}

    def build_unzeroed(c):
        module, trainer = build(c)
        g = torch.Generator().manual_seed(3)
        with torch.no_grad():
            for n, p in module.diffusion.named_parameters():
                if any(z in n for z in ("ssg1.", "ssg2.", "proj_out.", "u_mod.")):
                    p.copy_(torch.randn(p.shape, generator=g) * 0.02)
        module.diffusion_ema.module.load_state_dict(module.diffusion.state_dict())
        start.setdefault("weights", {k: v.detach().clone() for k, v in module.diffusion.state_dict().items()})
        return module, trainer

    monkeypatch.setattr(fit_mod, "build_from_config", build_unzeroed)
    module, trainer = fit_denoiser(str(path))
    train = [h["train/loss"] for h in trainer.history if "train/loss" in h]
    assert len(train) == STEPS and all(np.isfinite(train)) and all(x > 0 for x in train)
    val = [h for h in trainer.history if "val/loss" in h]
    assert len(val) == 1 and val[0]["val/loss"] > 0
    assert int(module.diffusion_ema.n_averaged) == STEPS
    # the decrease, on pinned draws
    files = sorted((tmp_path / "data").glob("*/0.latent.npz"))[2:5]             # three of the six training maps (the first two are held out)
    bt = collate_ragged([load_latents(f) for f in files], 64)
    t, x0 = torch.tensor([0.2, 0.5, 0.8]), torch.randn(bt.z.shape, generator=torch.Generator().manual_seed(5))
    end = {k: v.detach().clone() for k, v in module.diffusion.state_dict().items()}

    def pinned_loss(weights):
        module.diffusion.load_state_dict(weights)
        with torch.no_grad(), trainer._autocast(dev):
            loss, _ = module(module.diffusion, bt.h.to(dev), bt.z.to(dev), bt.s.to(dev), None, lengths=bt.lengths, t=t.to(dev), x0=x0.to(dev))
        return float(loss)

    before, after = pinned_loss(start["weights"]), pinned_loss(end)
    print(f"MEASURED ragged fit, pinned batch: {before:.4f} -> {after:.4f} after {STEPS} steps")
    assert np.isfinite(before) and np.isfinite(after) and after < 0.95 * before, (before, after)
    ck = tmp_path / "run" / "checkpoints" / "best.ckpt"
    state = torch.load(ck, map_location="cpu", weights_only=False)
    assert "diffusion.proj_in.weight" in state["state_dict"] and "diffusion_ema.n_averaged" in state["state_dict"]
    module.load_state_dict(state["state_dict"])
    # resume from it, still ragged
    cfg["trainer"].update(max_steps=STEPS + 1, val_check_interval=None, max_epochs=1)
    path.write_text(yaml.safe_dump(cfg))
    _, trainer2 = fit_denoiser(str(path), ckpt_path=str(ck))
    assert trainer2.global_step >= STEPS + 1
    lines = [json.loads(l) for l in open(tmp_path / "run" / "metrics.jsonl")]
    assert any(l.get("step") == STEPS + 1 and np.isfinite(l["train/loss"]) for l in lines)


def test_fit_denoiser_ragged_refuses_two_devices(dev, tmp_path):
    cfg = _ragged_cfg(tmp_path, dev)
    cfg["trainer"]["devices"] = 2
    path = tmp_path / "ragged2.yml"
    path.write_text(yaml.safe_dump(cfg))
    with pytest.raises(RuntimeError, match="ragged training .* runs on one device"):
        fit_denoiser(str(path))


# ---------------------------------------------------------------- 6. the no-grad varlen forward is what it was
@pytest.mark.parametrize("dt", [None, torch.bfloat16], ids=["fp32", "bf16"])
def test_nograd_forward_with_lengths_is_untouched(dev, dt):
    """forward(..., lengths=) under no_grad: each song as `forward` gives it alone (test_sample_many.py's check, on the tiny model), the same
    bits before and after a ragged training step on the same model, and with grad enabled the same values with a backward."""
    d = _dims(32, 2)
    P = O.init_params(d, seed=91)
    for k in P:
        if any(z in k for z in ("ssg1.", "ssg2.", "proj_out.", "u_mod.")):
            P[k] = torch.randn(P[k].shape, generator=torch.Generator().manual_seed(len(k))) * 0.05
    data = O.synthetic_batch(d, len(LENS), LPAD, seed=92)
    tr = make_trainer(d, P, dev)
    m = tr.diffusion
    m.compute_dtype = dt
    h, s = data["h"].clone(), data["s"].to(dev)
    xt = torch.lerp(data["x0"], data["z"], data["t"][:, None, None])
    for b, Lb in enumerate(LENS):
        h[b, :, Lb:] = 0
        xt[b, :, Lb:] = 0
    h, xt = h.to(dev), xt.to(dev)
    with torch.no_grad():
        u, v = m(h, s, xt, lengths=LENS)
        bound = 1e-3 if dt is not None else 1e-5
        for b, Lb in enumerate(LENS):
            u1, v1 = m(h[b:b + 1, :, :Lb].contiguous(), s[b:b + 1], xt[b:b + 1, :, :Lb].contiguous())
            assert rel_l2(u[b:b + 1], u1) <= bound and rel_l2(v[b:b + 1, :, :Lb], v1) <= bound, (b, Lb)
            assert torch.count_nonzero(v[b, :, Lb:]).item() == 0
    assert not m.engine.train
    step(tr, data, dev, lengths=LENS)                         # a ragged training step in between re-plans with train=True
    with torch.no_grad():
        u2, v2 = m(h, s, xt, lengths=LENS)
    # (v: row-wise kernels, no atomics; u's frame sum is accumulated with fp32 atomics, whose order is free outside OD_DETERMINISTIC)
    assert torch.equal(v.view(torch.int32), v2.view(torch.int32)) and rel_l2(u2, u) <= 1e-6
    m.eval()                                                  # eval mode with grad enabled still refuses, as before ragged training existed
    with pytest.raises(RuntimeError, match="has no backward in eval mode"):
        m(h, s, xt, lengths=LENS)
    m.train()
    ug, vg = m(h, s, xt, lengths=LENS)                        # grad enabled, training mode: the ragged training forward
    assert ug.requires_grad and vg.requires_grad and m.engine.train and m.engine.varlen
    assert rel_l2(ug, u) <= bound and rel_l2(vg, v) <= bound and torch.count_nonzero(vg[0, :, LENS[0]:]).item() == 0
    (ug.sum() + (vg * vg).sum()).backward()
    assert bool(torch.isfinite(m.arena.grad).all()) and float(m.arena.grad.abs().max()) > 0
