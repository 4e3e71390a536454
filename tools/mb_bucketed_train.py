"""What frame-budget, length-bucketed batches buy over fixed-count ragged batches: one training epoch (every step: zero_grad, forward,
backward, clip + AdamW + EMA — fit.Trainer.train_group) of the default denoiser (model.yml: depth 8, D = 512, 16 heads of 64; 46.9 M
parameters) in bf16 over a synthetic set of whole maps of 300 .. 1500 latent frames (the lengths of profiles/r12_ragged_train.txt), in one
process:

  fixed_count     LatentDataModule(seq_len=None, batch_size=8): the next eight maps of the stream, padded to the longest
  bucketed_cacheN the same maps with batch_frames = the mean padded frames (B * Lpad) per step of fixed_count: maps of similar length share a
                  batch, so (B, Lpad) changes from step to step.  N = how many training plans the engine keeps (OD_PLAN_CACHE): 1 is the
                  engine as it was — every change of (B, Lpad) allocates and zero-fills a new workspace and re-derives the RoPE table.
                  The difference between the bucketed legs is what the plan switches cost.

Every leg runs on a trainer of its own holding the same weights.  The epoch's batches are collated once and moved to the device before
anything is timed, so the figures are the steps' kernel, launch and planning time, not the loader's.  Each leg's epoch is run once untimed
(every shape's first launches), then the legs alternate within each repetition; times are host clocks around an epoch that ends in a device
synchronise.  The record carries the library's source hash and a bare-MFMA calibration of the box (bench.mfma_calibration) taken before and
after.  Expectations to report against: the bucketed legs' padding efficiency sum(lengths) / sum(B * Lpad) is strictly higher than
fixed_count's, and their valid frames per second at least fixed_count's.

  python tools/mb_bucketed_train.py [--maps 256] [--reps 5] [--out profiles/r13_bucketed_train.txt]
"""
import argparse
import json
import os
import statistics
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from oracle import denoiser_oracle as O  # noqa: E402
from osu_dreamer_amd import _lib  # noqa: E402
from osu_dreamer_amd.data import LatentDataModule, RaggedLatentBatch, write_synthetic_dataset  # noqa: E402
from osu_dreamer_amd.fit import Trainer  # noqa: E402
from osu_dreamer_amd.lr_schedule import LRScheduleArgs  # noqa: E402
from osu_dreamer_amd.model import BackboneArgs, DiffusionModelArgs  # noqa: E402
from osu_dreamer_amd.train import DiffusionTrainer  # noqa: E402

HELD_OUT, FIXED_B, PAD, MAX_LEN, BUCKET_POOL = 8, 8, 64, 1536, 128


def lengths_of(n_maps):
    """`n_maps` lengths spread evenly over 300 .. 1500 frames, in a scrambled (seeded) order: the stream is not sorted by length."""
    lens = [300 + round(i * 1200 / (n_maps - 1)) for i in range(n_maps)]
    perm = torch.randperm(n_maps, generator=torch.Generator().manual_seed(13)).tolist()
    return [lens[i] for i in perm]


def epoch_batches(data_path, **data_args):
    torch.manual_seed(0)
    dm = LatentDataModule(seq_len=None, num_workers=0, max_val_count=HELD_OUT, max_val_frac=.3, data_path=data_path, max_len=MAX_LEN,
                          pad_multiple=PAD, **data_args)
    return list(dm.train_dataloader())


def shape_stats(batches):
    valid = sum(int(b.lengths.sum()) for b in batches)
    padded = sum(b.z.shape[0] * b.z.shape[-1] for b in batches)
    keys = sorted({(b.z.shape[0], b.z.shape[-1]) for b in batches})
    return {"steps": len(batches), "songs": sum(b.z.shape[0] for b in batches), "valid_frames": valid, "padded_frames": padded,
            "padding_efficiency": round(valid / padded, 4), "mean_padded_frames_per_step": round(padded / len(batches), 1),
            "distinct_B_Lpad": len(keys), "B_Lpad": keys}


def make_trainer(d, P, dev):
    tr = DiffusionTrainer(val_batches=2, opt_args=dict(lr=3e-4, weight_decay=0.01),
                          schedule_args=LRScheduleArgs(warmup_init=.3, warmup_steps=1000, decay_start=30000),
                          osl_weight=1., del_weight=30., emb_dim=d.emb_dim, a_dim=d.a_dim, style_dim=d.style_dim,
                          diffusion_args=DiffusionModelArgs(d.global_cond_dim, d.backbone_dim,
                                                            BackboneArgs(d.depth, d.expand, d.head_dim, d.n_heads, d.radius), d.u_head_dim))
    tr.diffusion.load_state_dict(P)
    tr.diffusion_ema.module.load_state_dict(P)
    tr = tr.to(dev)
    tr.diffusion.compute_dtype = torch.bfloat16
    tr.gradient_clip_val = 1.0
    cfg = tr.configure_optimizers()
    return tr, cfg["optimizer"], cfg["lr_scheduler"]["scheduler"]


class Leg:
    def __init__(self, name, batches, d, P, dev, plan_cache, root):
        self.name, self.dev, self.plan_cache = name, dev, plan_cache
        self.batches = [RaggedLatentBatch(*(t.to(dev) for t in b[:4]), b.lengths) for b in batches]
        self.stats = shape_stats(batches)
        self.module, self.opt, self.sched = make_trainer(d, P, dev)
        self.trainer = Trainer(precision="bf16-mixed", default_root_dir=root, enable_checkpointing=False)
        self.times, self.loss = [], None

    def epoch(self):
        """One epoch; returns (seconds, plan switches, workspaces built)."""
        os.environ["OD_PLAN_CACHE"] = str(self.plan_cache)
        eng = self.module.diffusion.engine
        s0, b0 = eng.plan_switches, eng.plan_builds
        sync = torch.cuda.synchronize if self.dev.type == "cuda" else (lambda: None)
        sync()
        t = time.perf_counter()
        for i, b in enumerate(self.batches):
            self.trainer.train_group(self.module, self.opt, self.sched, [b], self.dev, i)
        sync()
        dt = time.perf_counter() - t
        self.loss = float(self.module._logged["train/loss"])
        return dt, eng.plan_switches - s0, eng.plan_builds - b0


def calibration(dev):
    try:
        import bench
        return bench.mfma_calibration(dev)
    except Exception as e:          # the record says so rather than carrying no calibration silently
        return {"error": repr(e)}


def run(dev, n_maps=256, reps=5, depth=8, dims=None, caches=(1, 8, 16), calibrate=True):
    d = dims or O.Dims(depth=depth)
    P = O.init_params(d, seed=1)
    lens = lengths_of(n_maps + HELD_OUT)
    with tempfile.TemporaryDirectory() as tmp:
        write_synthetic_dataset(os.path.join(tmp, "data"), n_maps=len(lens), frames=lens, a_dim=d.a_dim, emb_dim=d.emb_dim,
                                style_dim=d.style_dim, seed=2)
        fixed = epoch_batches(os.path.join(tmp, "data"), batch_size=FIXED_B)
        budget = int(round(sum(b.z.shape[0] * b.z.shape[-1] for b in fixed) / len(fixed)))
        bucketed = epoch_batches(os.path.join(tmp, "data"), batch_size=64, batch_frames=budget, bucket_pool=BUCKET_POOL)
        cal0 = calibration(dev) if calibrate else None
        legs = [Leg("fixed_count", fixed, d, P, dev, 1, tmp)] + [Leg(f"bucketed_cache{n}", bucketed, d, P, dev, n, tmp) for n in caches]
        warm = {leg.name: leg.epoch() for leg in legs}                 # every shape's first launches, and the caches' first fill
        plans = {}
        for _ in range(reps):
            for leg in legs:
                dt, switches, builds = leg.epoch()
                leg.times.append(dt)
                plans[leg.name] = {"plan_switches_per_epoch": switches, "workspaces_built_per_epoch": builds}
        cal1 = calibration(dev) if calibrate else None
    out = {}
    for leg in legs:
        med = statistics.median(leg.times)
        ws = leg.module.diffusion.engine._plans
        out[leg.name] = {**{k: v for k, v in leg.stats.items() if k != "B_Lpad"}, "epoch_s": [round(t, 4) for t in leg.times],
                         "epoch_s_median": round(med, 4), "ms_per_step_median": round(med / leg.stats["steps"] * 1e3, 2),
                         "valid_frames_per_s": round(leg.stats["valid_frames"] / med), **plans[leg.name],
                         "warm_up_epoch_s": round(warm[leg.name][0], 3), "cached_workspaces": len(ws),
                         "cached_workspace_bytes": sum(w.bytes for w in ws.values()), "last_loss": round(leg.loss, 4)}
    a = out["fixed_count"]
    best = max((n for n in out if n != "fixed_count"), key=lambda n: out[n]["valid_frames_per_s"])
    uncached, cached = out[f"bucketed_cache{caches[0]}"], out[f"bucketed_cache{caches[-1]}"]
    return {"tool": "mb_bucketed_train", "kernel_src_sha": _lib.source_sha(), "device": torch.cuda.get_device_name(0) if dev.type == "cuda" else "cpu",
            "dtype": "bf16", "model": f"model.yml defaults, depth {d.depth}", "training_maps": n_maps, "lengths": "300 .. 1500, evenly spread, scrambled",
            "what": "one epoch of full training steps (zero_grad, forward, backward, clip + AdamW + EMA) on batches resident on the device",
            "batch_frames": budget, "bucket_pool": BUCKET_POOL, "bucketed_B_Lpad": legs[1].stats["B_Lpad"], "legs": out,
            "plan_switch_ms_per_switch": round((uncached["epoch_s_median"] - cached["epoch_s_median"]) * 1e3
                                               / max(1, uncached["workspaces_built_per_epoch"] - cached["workspaces_built_per_epoch"]), 3),
            "expectation_padding_efficiency_higher": bool(out[best]["padding_efficiency"] > a["padding_efficiency"]),
            "expectation_valid_frames_per_s_at_least": {n: bool(v["valid_frames_per_s"] >= a["valid_frames_per_s"]) for n, v in out.items()
                                                        if n != "fixed_count"},
            "valid_frames_per_s_over_fixed_count": {n: round(v["valid_frames_per_s"] / a["valid_frames_per_s"], 3) for n, v in out.items()
                                                    if n != "fixed_count"},
            "calibration_before": cal0, "calibration_after": cal1}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--maps", type=int, default=256, help="training maps in the epoch")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--depth", type=int, default=8)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r13_bucketed_train.txt"), help="the record is appended to this file")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("mb_bucketed_train measures on an MI355X: no GPU is visible")
    _lib.lib()
    rec = run(torch.device("cuda:0"), n_maps=args.maps, reps=args.reps, depth=args.depth)
    line = json.dumps(rec)
    print(line, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "a") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
