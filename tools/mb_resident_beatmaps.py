"""How much of a `fit-latent` epoch waits for the host loader, and what the resident beatmap feed (osu_dreamer_amd/resident.py) does to it.

Whole epochs, FEED INCLUDED, of full training steps (zero_grad, forward, backward, clip + AdamW — fit.Trainer.train_group on the
LatentTrainer of the shipped latent.yml: batch 32 x 2052 frames, max_per_map 1, bf16) on a write_synthetic_beatmaps tree with realistic
map lengths (10 000 .. 50 000 frames, two difficulties per mapset).  Three legs on trainers of their own holding the same weights:

  loader_w0    BeatmapDataModule, num_workers 0
  loader_w13   BeatmapDataModule, num_workers 13 (the shipped value; 13 loader processes beside the trainer, never more)
  resident     ResidentBeatmapDataModule

A loader leg builds its DataLoader anew every epoch, as fit.Trainer does.  Method (tools/mb_resident_feed.py's): the legs alternate within
each repetition in one process, one untimed epoch each first, medians of `--reps` epochs, host clocks around an epoch that ends in a device
synchronise, a bare-MFMA calibration before and after, the library's source hash.  Every epoch runs under a time limit of its own
(`--leg-timeout` seconds, checked after every step): a leg that exceeds it is reported as timed out and leaves the rotation.

Every epoch is split at its first batch: `first_batch_s` is the time from asking for the iterator to holding the first batch — for the
13-worker leg the start of its processes plus one batch per worker's own shard — and `sustained_samples_per_s` counts the samples after
the first batch over the time after it, so what the workers sustain is reported apart from what starting them costs.  The resident leg adds
the gather's own time per batch (descriptor copy, three od_feed_gather_quant launches, the labels' index_select).

  python tools/mb_resident_beatmaps.py [--maps 1024] [--reps 5] [--out profiles/r15_resident_beatmaps.txt]
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
import yaml  # noqa: E402

from osu_dreamer_amd import _lib  # noqa: E402
from osu_dreamer_amd.data import BeatmapDataModule, write_synthetic_beatmaps  # noqa: E402
from osu_dreamer_amd.fit import DEFAULT_LATENT_CONFIG, build_latent_from_config  # noqa: E402
from osu_dreamer_amd.resident import ResidentBeatmapDataModule  # noqa: E402
from tools.mb_bucketed_train import calibration  # noqa: E402

WORKERS = (0, 13)             # fixed: never sized by the machine's CPU count, never more than 13 loader processes beside the trainer
HELD_OUT, MAPS_PER_SET = 64, 2


def lengths_of(n_mapsets):
    """`n_mapsets` lengths spread evenly over 10 000 .. 50 000 frames (1 .. 5 minutes at 6 ms a frame), in a scrambled (seeded) order."""
    lens = [10000 + round(i * 40000 / max(n_mapsets - 1, 1)) for i in range(n_mapsets)]
    perm = torch.randperm(n_mapsets, generator=torch.Generator().manual_seed(13)).tolist()
    return [lens[i] for i in perm]


class LegTimeout(Exception):
    pass


class Leg:
    def __init__(self, name, dm, module, opt, sched, trainer, dev, limit):
        self.name, self.dm, self.dev, self.limit = name, dm, dev, limit
        self.module, self.opt, self.sched, self.trainer = module, opt, sched, trainer
        self.runs, self.warm, self.dead = [], None, None

    def epoch(self):
        """One epoch, feed included: dict(seconds, seconds to the first batch, seconds inside the steps' spans, samples, steps)."""
        loader = self.dm.train_dataloader()
        spans, samples, first_samples, i, t_first = [], 0, 0, 0, None
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        it = iter(loader)
        while True:
            batch = next(it, None)
            if batch is None:
                break
            if t_first is None:
                t_first, first_samples = time.perf_counter() - t0, int(batch[2].shape[0])
            batch = self.trainer._to(batch, self.dev)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            self.trainer.train_group(self.module, self.opt, self.sched, [batch], self.dev, i)
            e1.record()
            spans.append((e0, e1))
            samples += int(batch[2].shape[0])
            i += 1
            if time.perf_counter() - t0 > self.limit:
                del it, loader
                raise LegTimeout(f"{self.name}: an epoch passed {self.limit} s at step {i}")
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        del it, loader                           # a loader leg's workers end here: at most 13 are alive at a time
        return dict(s=dt, first=t_first or 0.0, inside=sum(a.elapsed_time(b) for a, b in spans) * 1e-3, samples=samples,
                    after_first=samples - first_samples, steps=i)


def make_legs(data_path, dev, root, limit):
    cfg = yaml.safe_load(open(DEFAULT_LATENT_CONFIG))
    cfg["trainer"].update(default_root_dir=root, enable_checkpointing=False)
    data = {k: v for k, v in cfg["data"].items() if k != "num_workers"}
    data.update(max_val_count=HELD_OUT, data_path=data_path)
    legs, state = [], None
    for name, dm in [(f"loader_w{w}", BeatmapDataModule(num_workers=w, **data)) for w in WORKERS] + \
                    [("resident", ResidentBeatmapDataModule(num_workers=0, device=dev, **data))]:
        module, trainer = build_latent_from_config(cfg)
        state = state or {k: v.clone() for k, v in module.state_dict().items()}
        module.load_state_dict(state)
        module.gradient_clip_val = trainer.gradient_clip_val
        module.to(dev)
        oc = module.configure_optimizers()
        legs.append(Leg(name, dm, module, oc["optimizer"], oc["lr_scheduler"]["scheduler"], trainer, dev, limit))
    return legs, data


def gather_times(leg):
    """The resident leg's gather alone over one planned epoch: the whole gather of a batch as a device span, and the host's time to launch it."""
    feed = leg.dm.train_dataloader()
    plan = feed.plan_epoch()
    if not plan:
        return {"batches": 0}
    for pb in plan[:2]:
        feed.gather(pb)
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0 = time.perf_counter()
    e0.record()
    for pb in plan:
        feed.gather(pb)
    e1.record()
    host = time.perf_counter() - t0
    torch.cuda.synchronize()
    B, T = len(plan[0].maps), plan[0].Lpad
    us = e0.elapsed_time(e1) * 1e3 / len(plan)
    moved = B * T * (72 + 7 + 4) + 4 * B * T * (72 + 9)          # bytes read + bytes written
    return {"batches": len(plan), "batch_shape": [B, 72 + 9, T], "gather_us_per_batch_device_span": round(us, 1),
            "gather_us_per_batch_host_launch": round(host * 1e6 / len(plan), 1), "gather_GBps_over_the_span": round(moved / us * 1e-3, 1)}


def summarise(legs):
    out = {}
    for leg in legs:
        if leg.dead or not leg.runs:
            out[leg.name] = {"timed_out": leg.dead}
            continue
        med = statistics.median(r["s"] for r in leg.runs)
        r0 = leg.runs[0]
        sustained = [r["after_first"] / (r["s"] - r["first"]) for r in leg.runs if r["after_first"] > 0 and r["s"] > r["first"]]
        out[leg.name] = {"epoch_s": [round(r["s"], 3) for r in leg.runs], "epoch_s_median": round(med, 3), "warm_up_epoch_s": round(leg.warm, 3),
                         "steps": r0["steps"], "samples": r0["samples"], "samples_per_s": round(r0["samples"] / med, 1),
                         "ms_per_step_median": round(med / max(r0["steps"], 1) * 1e3, 2),
                         "first_batch_s": [round(r["first"], 3) for r in leg.runs],
                         "first_batch_s_median": round(statistics.median(r["first"] for r in leg.runs), 3),
                         "sustained_samples_per_s": round(statistics.median(sustained), 1) if sustained else None,
                         "outside_steps_fraction": round(statistics.median(1.0 - r["inside"] / r["s"] for r in leg.runs), 4)}
    res = out.get("resident", {})
    for key in ("samples_per_s", "sustained_samples_per_s"):
        if res.get(key):
            out[f"resident_over_loader_{key}"] = {n: round(res[key] / v[key], 3) for n, v in out.items()
                                                   if n.startswith("loader_") and isinstance(v, dict) and v.get(key)}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--maps", type=int, default=1024, help="training maps (two per mapset)")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--leg-timeout", type=float, default=150.0, help="seconds one epoch of one leg may take")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r15_resident_beatmaps.txt"), help="the record is appended to this file")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("mb_resident_beatmaps measures on an MI355X: no GPU is visible")
    _lib.lib()
    dev = torch.device("cuda:0")
    rec = {"tool": "mb_resident_beatmaps", "kernel_src_sha": _lib.source_sha(), "device": torch.cuda.get_device_name(0), "dtype": "bf16",
           "model": "latent.yml defaults", "reps": args.reps, "loader_workers": list(WORKERS),
           "what": "whole fit-latent epochs of full training steps, feed included; a loader leg builds its DataLoader every epoch, as fit.Trainer does",
           "calibration_before": calibration(dev)}
    with tempfile.TemporaryDirectory() as tmp:
        n_sets = (args.maps + HELD_OUT) // MAPS_PER_SET
        t0 = time.perf_counter()
        write_synthetic_beatmaps(os.path.join(tmp, "data"), n_mapsets=n_sets, maps_per_set=MAPS_PER_SET, frames=lengths_of(n_sets), seed=2)
        rec["dataset"] = {"mapsets": n_sets, "maps_per_set": MAPS_PER_SET, "held_out_maps": HELD_OUT,
                          "lengths": "10000 .. 50000 frames, evenly spread, scrambled", "write_s": round(time.perf_counter() - t0, 1)}
        print(json.dumps(rec["dataset"]), flush=True)
        torch.manual_seed(0)
        t0 = time.perf_counter()
        legs, data = make_legs(os.path.join(tmp, "data"), dev, tmp, args.leg_timeout)
        res = legs[-1]
        rec["data_args"] = {k: v for k, v in data.items() if k != "data_path"}
        rec["resident_store"] = {"bytes": res.dm.store.nbytes, "maps": len(res.dm.store), "build_s_with_the_three_trainers": round(time.perf_counter() - t0, 1)}
        print(json.dumps(rec["resident_store"]), flush=True)
        for rep in range(args.reps + 1):                 # repetition 0: one untimed epoch each (first launches, workspaces, the page cache)
            for leg in legs:
                if leg.dead:
                    continue
                try:
                    r = leg.epoch()
                except LegTimeout as e:
                    leg.dead = str(e)
                    print(json.dumps({"rep": rep, "leg": leg.name, "timed_out": leg.dead}), flush=True)
                    continue
                if rep == 0:
                    leg.warm = r["s"]
                else:
                    leg.runs.append(r)
                print(json.dumps({"rep": rep, "leg": leg.name, **{k: round(v, 3) if isinstance(v, float) else v for k, v in r.items()}}), flush=True)
        rec["legs"] = summarise(legs)
        rec["od_feed_gather_quant"] = gather_times(res)
        del legs, res
    rec["calibration_after"] = calibration(dev)
    line = json.dumps(rec)
    print(line, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "a") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
