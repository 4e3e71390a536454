"""Gradient accumulation: fit.Trainer(accumulate_grad_batches=k) and Trainer.train_group.

An optimizer step on micro-batches of B_1 .. B_m songs scales micro-batch i's loss by B_i / sum(B), so the accumulated gradient is the mean
over all the songs — what one step on the union batch computes:
  5. a ragged group (Lpads 192, 64, 128) against ONE ragged step on its six songs and against the mean of the six single-song dense steps;
  6. a dense group (3 x B = 2) against one dense step on B = 6;
  7. the bookkeeping through `fit-denoiser`: optimizer steps, EMA updates, the LR schedule and the epoch's last, shorter group;
  8. k = 1 is the plain step, bit for bit (weights, EMA, AdamW moments);
  9. data parallel (gloo, world 2, the emulator): each bucket is exchanged once per optimizer step, the ranks agree, and the step is the
     oracle's on the mean of the four per-(rank, micro-batch) gradients;
 10. fit-style / fit-latent refuse the key instead of dropping it.
The kernel-running tests run on the emulator and on the MI355X (the `dev` fixture), test 9 on the emulator only (gloo).
"""
import json
import math
import os
import sys

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp
import yaml

from oracle import denoiser_oracle as O
from osu_dreamer_amd import det
from osu_dreamer_amd import fit as fit_mod
from osu_dreamer_amd.data import RaggedLatentBatch
from osu_dreamer_amd.fit import (DEFAULT_LATENT_CONFIG, DEFAULT_STYLE_CONFIG, Trainer, build_latent_from_config, build_style_from_config,
                                 fit_denoiser)
from kernel_backend import dev  # noqa: F401
from test_ddp_gloo import REPO, _free_port
from test_model_parity import make_trainer
from test_ragged_train import EPS, _dims, _mean_of_single_steps, _ragged_cfg, step

LOGS = ("loss", "osl", "del", "u_mape")


def pin_draws(tr, data, dev):
    """Every forward of `tr` takes its songs' t and x0 from `data` (the songs are recognised by their style vectors), so that a song gets
    the same draws in whichever batch it is stepped."""
    forward = tr.forward

    def pinned(model, h, x1, s, labels=None, *, lengths=None, t=None, x0=None):
        rows = [next(i for i in range(data["s"].shape[0]) if torch.equal(data["s"][i], s[b].cpu())) for b in range(s.shape[0])]
        return forward(model, h, x1, s, labels, lengths=lengths, t=data["t"][rows].to(dev),
                       x0=data["x0"][rows][..., :x1.shape[-1]].contiguous().to(dev))
    tr.forward = pinned


def micro_batch(data, rows, dev, Lpad=None, lengths=None):
    h, z, s = (data[k][rows] for k in ("h", "z", "s"))
    if lengths is None:
        return (h.to(dev), z.to(dev), s.to(dev), torch.zeros(len(rows), 5, device=dev))
    return RaggedLatentBatch(h[..., :Lpad].contiguous().to(dev), z[..., :Lpad].contiguous().to(dev), s.to(dev),
                             torch.zeros(len(rows), 5, device=dev), torch.tensor(lengths))


def run_group(tr, batches, dev, tmp_path, hold_step=True):
    """Trainer.train_group on `batches`; with `hold_step` the optimizer's step is left out, so the arena keeps the weights and the gradient."""
    trainer = Trainer(precision="32", default_root_dir=str(tmp_path), enable_checkpointing=False, accumulate_grad_batches=len(batches))
    cfg = tr.configure_optimizers()
    opt, sched = cfg["optimizer"], cfg["lr_scheduler"]["scheduler"]
    if hold_step:
        opt.step = lambda *a, **k: None
    logs = trainer.train_group(tr, opt, sched, batches, dev)
    assert trainer.global_step == 1
    return {k[len("train/"):]: float(v) for k, v in logs.items()}, {k: p.grad.detach().cpu().clone() for k, p in tr.diffusion.named_parameters()}


def unzeroed(d, seed):
    P = O.init_params(d, seed=seed)
    for k in P:                                   # (the reference zero-initialises these: un-zero them so every gradient is live)
        if any(z in k for z in ("ssg1.", "ssg2.", "proj_out.", "u_mod.")):
            P[k] = torch.randn(P[k].shape, generator=torch.Generator().manual_seed(len(k))) * 0.05
    return P


def dist_of(a, b):
    return {k: float((a[k].double() - b[k].double()).norm() / (b[k].double().norm() + 1e-300)) for k in a}


# ---------------------------------------------------------------- 5. ragged group = union step
GROUP = [((130, 65, 1), 192), ((64,), 64), ((40, 96), 128)]
UNION = [n for lens, _ in GROUP for n in lens]


@pytest.mark.parametrize("dt", [None, torch.bfloat16], ids=["fp32", "bf16"])
def test_ragged_group_is_the_union_step(dev, dt, tmp_path):
    """Micro-batches of lengths (130, 65, 1), (64,), (40, 96) — Lpads 192, 64, 128, weights 3/6, 1/6, 2/6 — through Trainer.train_group, the
    gradient read before the optimizer step, against ONE ragged step on the six songs in Lpad = 192 and against the mean of the six dense
    single-song steps, per parameter tensor and relative to the gradient's norm.  The yardstick is measured here with the existing code
    paths alone: the distance between that mean and that one ragged step.  Bound: 4 x the yardstick and at least 8 eps of the compute dtype.
    The logged loss / osl / del / u_mape equal the union step's within 1e-5 (fp32) / 1e-4 (bf16) relative, as the ragged step is held to the
    single-song steps in test_ragged_train.py.
    Measured, worst tensor (emulator | MI355X): fp32 group against union 2.7e-7 | 1.7e-7, against the single-song mean 4.6e-7 | 4.2e-7,
    yardstick 4.5e-7 | 4.5e-7 (bound 1.8e-6 on that tensor, 9.5e-7 = 8 eps at least); bf16 group against union 2.5e-4 | 1.1e-7, against the
    single-song mean 5.9e-3 | 5.9e-3, yardstick 5.9e-3 | 5.9e-3 (bound 6.2e-2 = 8 eps of bf16).  Loss: equal to the union step's to the
    printed six decimals in every case."""
    d = _dims(32, 2, 2, 1)
    P = unzeroed(d, 111)
    data = O.synthetic_batch(d, len(UNION), 192, seed=112)
    # existing code only: one ragged step on the union, and the mean of the single-song dense steps
    tr = make_trainer(d, P, dev)
    tr.diffusion.compute_dtype = dt
    ul, ulogs, ug, _ = step(tr, data, dev, lengths=UNION)
    sl, slogs, sg = _mean_of_single_steps(d, P, data, dev, dt, UNION)
    margin = dist_of(ug, sg)
    # the group
    tr = make_trainer(d, P, dev)
    tr.diffusion.compute_dtype = dt
    pin_draws(tr, data, dev)
    batches, row = [], 0
    for lens, Lpad in GROUP:
        batches.append(micro_batch(data, list(range(row, row + len(lens))), dev, Lpad, list(lens)))
        row += len(lens)
    logs, gg = run_group(tr, batches, dev, tmp_path)
    assert tr.diffusion.engine.varlen
    rel = 1e-5 if dt is None else 1e-4
    for k in LOGS:
        assert logs[k] == pytest.approx(ulogs[k], rel=rel), k
        assert logs[k] == pytest.approx(slogs[k], rel=rel), k
    to_union, to_singles = dist_of(gg, ug), dist_of(gg, sg)
    print(f"MEASURED ragged group {'fp32' if dt is None else 'bf16'}: worst tensor against the union step {max(to_union.values()):.3e}, against the "
          f"single-song mean {max(to_singles.values()):.3e}, worst yardstick {max(margin.values()):.3e}; loss {logs['loss']:.6f} against {ul:.6f}")
    for k in gg:
        bound = max(4 * margin[k], 8 * EPS[dt])
        assert to_union[k] <= bound, f"{k}: group {to_union[k]:.3e} from the union step, bound {bound:.3e} (yardstick {margin[k]:.3e})"
        assert to_singles[k] <= bound, f"{k}: group {to_singles[k]:.3e} from the single-song mean, bound {bound:.3e} (yardstick {margin[k]:.3e})"


# ---------------------------------------------------------------- 6. dense group = one larger batch
@pytest.mark.parametrize("dt", [None, torch.bfloat16], ids=["fp32", "bf16"])
def test_dense_group_is_one_larger_batch(dev, dt, tmp_path):
    """k = 3 micro-batches of B = 2 x L = 24 (weights 1/3 each: Lightning's 1 / k) against one dense step on B = 6.  Batch linearity; the
    yardstick, existing code only: the distance between the mean of the six single-song dense steps and the one dense step on B = 6.
    Bound: 4 x that and at least 8 eps of the compute dtype.
    Measured, worst tensor (emulator | MI355X): fp32 4.6e-7 | 4.0e-7 against a yardstick of 5.2e-7 | 5.3e-7; bf16 9.9e-7 | 9.9e-8 against a
    yardstick of 6.6e-3 | 7.3e-3 (bound 6.2e-2 = 8 eps of bf16)."""
    d, B, L = O.TINY, 6, 24
    P = unzeroed(d, 121)
    data = O.synthetic_batch(d, B, L, seed=122)
    tr = make_trainer(d, P, dev)
    tr.diffusion.compute_dtype = dt
    bl, blogs, bg, _ = step(tr, data, dev)
    assert not tr.diffusion.engine.varlen
    _, _, sg = _mean_of_single_steps(d, P, data, dev, dt, [L] * B)
    margin = dist_of(bg, sg)
    tr = make_trainer(d, P, dev)
    tr.diffusion.compute_dtype = dt
    pin_draws(tr, data, dev)
    logs, gg = run_group(tr, [micro_batch(data, [2 * i, 2 * i + 1], dev) for i in range(3)], dev, tmp_path)
    assert not tr.diffusion.engine.varlen
    rel = 1e-5 if dt is None else 1e-4
    for k in LOGS:
        assert logs[k] == pytest.approx(blogs[k], rel=rel), k
    err = dist_of(gg, bg)
    print(f"MEASURED dense group {'fp32' if dt is None else 'bf16'}: worst tensor {max(err.values()):.3e}, worst yardstick {max(margin.values()):.3e}; "
          f"loss {logs['loss']:.6f} against {bl:.6f}")
    for k in gg:
        bound = max(4 * margin[k], 8 * EPS[dt])
        assert err[k] <= bound, f"{k}: group {err[k]:.3e} from the B = 6 step, bound {bound:.3e} (yardstick {margin[k]:.3e})"


# ---------------------------------------------------------------- 7. bookkeeping through fit-denoiser
def test_fit_denoiser_counts_optimizer_steps(dev, tmp_path, monkeypatch):
    """accumulate_grad_batches: 2 over an epoch of three batches (six training maps, batch_size 2): two optimizer steps, the second on one
    batch; the EMA was updated twice; metrics.jsonl has one record per optimizer step whose lr is the schedule's at that step."""
    cfg = _ragged_cfg(tmp_path, dev)
    cfg["data"].update(batch_size=2)
    cfg["model"]["opt_args"] = dict(lr=1e-3, weight_decay=0.0)
    cfg["model"]["schedule_args"] = dict(warmup_steps=4, warmup_init=0.25, decay_start=30000)
    cfg["trainer"].update(accumulate_grad_batches=2, max_epochs=1, max_steps=-1, val_check_interval=None, log_every_n_steps=1)
    path = tmp_path / "accumulate.yml"
    path.write_text(yaml.safe_dump(cfg))
    from osu_dreamer_amd.data import LatentDataModule
    n_batches = len(list(LatentDataModule(**cfg["data"]).train_dataloader()))
    assert n_batches == 3
    sizes, train_group = [], getattr(Trainer, "train_group", None)

    def recording(self, module, opt, sched, batches, device, batch_idx=0):
        sizes.append(len(batches))
        return train_group(self, module, opt, sched, batches, device, batch_idx)

    if train_group is not None:
        monkeypatch.setattr(Trainer, "train_group", recording)
    module, trainer = fit_denoiser(str(path))
    steps = math.ceil(n_batches / 2)
    assert trainer.global_step == steps
    assert int(module.diffusion_ema.n_averaged) == steps and module.diffusion_ema.count == steps
    assert sizes == [2, 1]
    lines = [json.loads(l) for l in open(tmp_path / "run" / "metrics.jsonl")]
    train = [l for l in lines if "train/loss" in l]
    assert [l["step"] for l in train] == list(range(1, steps + 1)) and all(np.isfinite(l["train/loss"]) for l in train)
    for l in train:
        assert l["lr"] == pytest.approx(1e-3 * 0.25 ** (1 - l["step"] / 4), rel=1e-12)
    assert len([l for l in lines if "val/loss" in l]) == 1 and trainer.epoch == 1


# ---------------------------------------------------------------- 8. k = 1 is the plain step
@pytest.mark.parametrize("ragged", [False, True], ids=["dense", "ragged"])
def test_group_of_one_is_the_plain_step(dev, ragged, tmp_path):
    """Two steps through train_group with one batch each against the sequence zero_grad; training_step; backward; step; sched.step;
    on_train_batch_end written out by hand, under OD_DETERMINISTIC: weights, EMA, AdamW moments and the learning rate bit-identical."""
    d = O.TINY
    P = unzeroed(d, 131)
    lens = [24, 17, 5]
    data = O.synthetic_batch(d, 3, 24, seed=132)
    out = []
    try:
        det.force(True)
        for grouped in (False, True):
            tr = make_trainer(d, P, dev)
            pin_draws(tr, data, dev)
            tr.gradient_clip_val = 1.0
            cfg = tr.configure_optimizers()
            opt, sched = cfg["optimizer"], cfg["lr_scheduler"]["scheduler"]
            trainer = Trainer(precision="32", default_root_dir=str(tmp_path), enable_checkpointing=False)
            for i in range(2):
                rows = [i, i + 1]
                batch = micro_batch(data, rows, dev, 24, [lens[r] for r in rows]) if ragged else micro_batch(data, rows, dev)
                if grouped:
                    trainer.train_group(tr, opt, sched, [batch], dev, i)
                else:
                    opt.zero_grad()
                    with trainer._autocast(dev):
                        loss = tr.training_step(batch, i)
                    loss.backward()
                    opt.step()
                    sched.step()
                    tr.on_train_batch_end()
            out.append([t.detach().cpu().clone() for t in (tr.diffusion.arena.data, tr.diffusion_ema.module.arena.data, opt.exp_avg,
                                                          opt.exp_avg_sq, tr.diffusion.arena.grad)]
                       + [opt.param_groups[0]["lr"], opt.step_count, tr.diffusion_ema.count, float(tr._logged["train/loss"])])
    finally:
        det.force(None)
    by_hand, grouped = out
    for a, b, what in zip(by_hand[:5], grouped[:5], ("weights", "EMA", "exp_avg", "exp_avg_sq", "gradient arena")):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32)), f"{what} differ between train_group and the hand-written step"
    assert by_hand[5:] == grouped[5:] and grouped[6] == 2 and grouped[7] == 2
    assert not torch.equal(grouped[0], grouped[1]), "the steps must have moved the weights off their average"


# ---------------------------------------------------------------- 9. data parallel
def _ddp_worker(rank, world, port, out_dir, tag):
    sys.path.insert(0, REPO)
    sys.path.insert(0, os.path.join(REPO, "tests"))
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK=str(rank))
    torch.set_num_threads(2)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    from osu_dreamer_amd import _lib
    from osu_dreamer_amd.ddp import GradBucketReducer
    from kernel_backend import EMU_SO
    _lib.use_library(EMU_SO)
    d = O.TINY
    P = O.init_params(d, seed=50 + rank)          # deliberately different: broadcast must fix it
    tr = make_trainer(d, P, torch.device("cpu"))
    red = GradBucketReducer(tr.diffusion)
    red.broadcast_parameters(0)
    tr.diffusion_ema.module.load_state_dict(tr.diffusion.state_dict())
    tr.gradient_clip_val = 1.0
    cfg = tr.configure_optimizers()
    opt, sched = cfg["optimizer"], cfg["lr_scheduler"]["scheduler"]
    trainer = Trainer(precision="32", devices=world, default_root_dir=out_dir, enable_checkpointing=False, accumulate_grad_batches=2)
    batches = []
    for j in range(2):
        data = O.synthetic_batch(d, 2, 24, seed=60 + 2 * rank + j)
        batches.append((data["h"], data["z"], data["s"], torch.zeros(2, 5)))
    draws = {k: torch.cat([O.synthetic_batch(d, 2, 24, seed=60 + 2 * rank + j)[k] for j in range(2)]) for k in ("s", "t", "x0")}
    pin_draws(tr, draws, torch.device("cpu"))
    exchanged_early = []
    reduce = red._reduce

    def watching(g):
        exchanged_early.append(red._deferred)
        return reduce(g)
    red._reduce = watching
    trainer.train_group(tr, opt, sched, batches, torch.device("cpu"))
    torch.save({"p": tr.diffusion.arena.data.clone(), "ema": tr.diffusion_ema.module.arena.data.clone(),
                "g": tr.diffusion.arena.grad.clone(), "buckets": list(red.bucket_log), "early": exchanged_early,
                "steps": (trainer.global_step, opt.step_count, tr.diffusion_ema.count)}, os.path.join(out_dir, f"{tag}rank{rank}.pt"))
    dist.destroy_process_group()


@pytest.mark.parametrize("det_mode", ["0", "1"])
def test_data_parallel_group_exchanges_once(tmp_path, det_mode, monkeypatch):
    """World 2, each rank accumulates k = 2 micro-batches of B = 2 x L = 24 (fixed windows): the ranks end with identical weights / EMA /
    gradients, equal — within test_ddp_gloo.test_n_rank_step_matches_averaged_oracle's tolerances — to the oracle's step on the mean of the
    four per-(rank, micro-batch) gradients; every bucket was exchanged exactly once, after the first micro-batch's backward.  det_mode 1:
    the same under OD_DETERMINISTIC=1, and a second run gives the same bits."""
    from kernel_backend import build_emu
    build_emu()
    world = 2
    monkeypatch.setenv("OD_DETERMINISTIC", det_mode)          # the spawned ranks inherit it
    mp.spawn(_ddp_worker, args=(world, _free_port(), str(tmp_path), "a"), nprocs=world, join=True)
    r0, r1 = torch.load(tmp_path / "arank0.pt"), torch.load(tmp_path / "arank1.pt")
    assert torch.equal(r0["p"], r1["p"]) and torch.equal(r0["ema"], r1["ema"]) and torch.equal(r0["g"], r1["g"])
    assert r0["buckets"] == r1["buckets"] and r0["steps"] == r1["steps"] == (1, 1, 1)
    names = [n for n, _ in r0["buckets"]]
    assert len(names) == len(set(names)) >= 3 and sum(n for _, n in r0["buckets"]) == r0["g"].numel(), "every bucket once per optimizer step"
    assert names[0] == "tail" and names[-1] == "head"         # the usual completion order
    assert r0["early"] == [False] * len(names) and r1["early"] == r0["early"], "nothing may be exchanged inside the group"
    if det_mode == "1":
        mp.spawn(_ddp_worker, args=(world, _free_port(), str(tmp_path), "b"), nprocs=world, join=True)
        again = torch.load(tmp_path / "brank0.pt")
        for k in ("p", "ema", "g"):
            assert torch.equal(r0[k].view(torch.int32), again[k].view(torch.int32)), f"{k} differs from run to run under OD_DETERMINISTIC"

    from osu_dreamer_amd.model import DiffusionModel
    from test_model_parity import margs
    d = O.TINY
    P = O.init_params(d, seed=50)
    grads = []
    for rank in range(world):
        for j in range(2):
            data = O.synthetic_batch(d, 2, 24, seed=60 + 2 * rank + j)
            grads.append(O.loss_and_grads(P, d, data["h"], data["z"], data["s"], data["t"], data["x0"])[2])
    avg = {k: sum(g[k] for g in grads) / len(grads) for k in P}
    _, coef = O.clip_coef(avg, 1.0)
    m = {k: torch.zeros_like(v) for k, v in P.items()}
    vv = {k: torch.zeros_like(v) for k, v in P.items()}
    ema = {k: v.clone() for k, v in P.items()}
    Pc = {k: v.clone() for k, v in P.items()}
    O.adamw_ema_step(Pc, avg, m, vv, ema, 1, 3e-4 * O.lr_multiplier(0, 1000, .3, 30000), clip=coef, first_ema=True)
    model = DiffusionModel(d.emb_dim, d.a_dim, d.style_dim, margs(d))
    for k in P:
        assert torch.allclose(model.arena.view(k, r0["p"]), Pc[k], rtol=1e-4, atol=2e-6), k
        gg = model.arena.view(k, r0["g"])
        assert float((gg - avg[k]).norm() / (avg[k].norm() + 1e-12)) < 1e-3, k


# ---------------------------------------------------------------- 10. the other trainers
@pytest.mark.parametrize("config,build,command", [(DEFAULT_STYLE_CONFIG, build_style_from_config, "fit-style"),
                                                  (DEFAULT_LATENT_CONFIG, build_latent_from_config, "fit-latent")])
def test_other_trainers_refuse_accumulation(config, build, command):
    cfg = yaml.safe_load(open(config))
    cfg["trainer"]["accumulate_grad_batches"] = 2
    with pytest.raises(RuntimeError, match=f"accumulate_grad_batches=2 is not implemented for {command}"):
        build(cfg)
    cfg["trainer"]["accumulate_grad_batches"] = 1
    module, trainer = build(cfg)
    assert trainer.accumulate_grad_batches == 1 and trainer.global_step == 0
    del cfg["trainer"]["accumulate_grad_batches"]
    assert build(cfg)[1].accumulate_grad_batches == 1


def test_trainer_refuses_a_bad_count_and_a_group_on_another_module(tmp_path):
    with pytest.raises(ValueError, match="accumulate_grad_batches"):
        Trainer(default_root_dir=str(tmp_path), accumulate_grad_batches=0)
    module, trainer = build_style_from_config(yaml.safe_load(open(DEFAULT_STYLE_CONFIG)))
    with pytest.raises(RuntimeError, match="denoiser only"):
        trainer.train_group(module, None, None, [(), ()], torch.device("cpu"))
    assert fit_mod.build_from_config(yaml.safe_load(open(fit_mod.DEFAULT_CONFIG)))[1].accumulate_grad_batches == 1
