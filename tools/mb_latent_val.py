"""What one validation check of `fit-latent` costs, per map from the host loader and in ragged groups from a resident store
(`data.resident_val`, osu_dreamer_amd/resident.py: ResidentBeatmapValFeed; latent_train.py: LatentTrainer._validation_group).

Whole validation epochs — fit.Trainer.validate on the LatentTrainer of the shipped latent.yml, bf16 — over 64 held-out whole maps of
10 000 .. 50 000 frames written by write_synthetic_beatmaps, the feed included.  Legs, on one trainer (validation changes no state):

  host_w13        BeatmapDataModule.val_dataloader(), data.num_workers 13 as shipped (validation then reads through ONE worker process)
  host_w0         the same, num_workers 0: the maps are read in the trainer's process
  resident_<b>    ResidentBeatmapDataModule(resident_val=True, val_frame_budget=b): the default budget and two others

A host leg builds its DataLoader anew every epoch, as fit.Trainer.validate does; the resident legs build their store once, before the
first (untimed) epoch, and its build time is reported apart.  Method (tools/mb_resident_beatmaps.py's): the legs alternate within each
repetition in one process, one untimed epoch each first, medians and spreads (max - min) of `--reps` epochs, host clocks around an epoch
that ends in a device synchronise, a bare-MFMA calibration before and after, the library's source hash.  Every resident leg reports the
share of padded frames of each of its groups.

  python tools/mb_latent_val.py [--reps 5] [--out profiles/r16_latent_val.txt]
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
from osu_dreamer_amd.encode_latents import DEFAULT_FRAME_BUDGET  # noqa: E402
from osu_dreamer_amd.fit import DEFAULT_LATENT_CONFIG, build_latent_from_config  # noqa: E402
from osu_dreamer_amd.resident import ResidentBeatmapDataModule  # noqa: E402
from tools.mb_bucketed_train import calibration  # noqa: E402

WORKERS = (13, 0)             # fixed: never sized by the machine's CPU count
HELD_OUT, TRAIN = 64, 2       # one map per mapset; the two training maps only let the data modules be built
BUDGETS = (DEFAULT_FRAME_BUDGET, DEFAULT_FRAME_BUDGET // 4, DEFAULT_FRAME_BUDGET * 2)


def lengths_of(n):
    """`n` lengths spread evenly over 10 000 .. 50 000 frames (1 .. 5 minutes at 6 ms a frame), in a scrambled (seeded) order."""
    lens = [10000 + round(i * 40000 / max(n - 1, 1)) for i in range(n)]
    perm = torch.randperm(n, generator=torch.Generator().manual_seed(13)).tolist()
    return [lens[i] for i in perm]


class Leg:
    def __init__(self, name, dm):
        self.name, self.dm, self.runs, self.warm, self.dead, self.logs = name, dm, [], None, None, None

    def epoch(self, trainer, module, dev):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        self.logs = trainer.validate(module, self.dm, dev)
        torch.cuda.synchronize()
        return time.perf_counter() - t0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--leg-timeout", type=float, default=120.0, help="a leg whose epoch took longer leaves the rotation")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r16_latent_val.txt"), help="the record is appended to this file")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("mb_latent_val measures on an MI355X: no GPU is visible")
    _lib.lib()
    dev = torch.device("cuda:0")
    rec = {"tool": "mb_latent_val", "kernel_src_sha": _lib.source_sha(), "device": torch.cuda.get_device_name(0), "dtype": "bf16",
           "model": "latent.yml defaults", "reps": args.reps,
           "what": "whole validation epochs (fit.Trainer.validate) over the held-out maps, feed included",
           "calibration_before": calibration(dev)}
    with tempfile.TemporaryDirectory() as tmp:
        t0 = time.perf_counter()
        lens = lengths_of(HELD_OUT) + [10000] * TRAIN          # the hold-out rule takes the first mapsets of the sorted listing
        write_synthetic_beatmaps(os.path.join(tmp, "data"), n_mapsets=len(lens), maps_per_set=1, frames=lens, seed=2)
        rec["dataset"] = {"held_out_maps": HELD_OUT, "lengths": "10000 .. 50000 frames, evenly spread, scrambled",
                          "frames": sum(lens[:HELD_OUT]), "write_s": round(time.perf_counter() - t0, 1)}
        print(json.dumps(rec["dataset"]), flush=True)
        cfg = yaml.safe_load(open(DEFAULT_LATENT_CONFIG))
        cfg["trainer"].update(default_root_dir=tmp, enable_checkpointing=False)
        torch.manual_seed(0)
        module, trainer = build_latent_from_config(cfg)
        module.to(dev)
        data = {k: v for k, v in cfg["data"].items() if k not in ("num_workers", "resident", "resident_max_gb", "resident_val", "val_frame_budget")}
        data.update(max_val_count=HELD_OUT, max_val_frac=0.99, data_path=os.path.join(tmp, "data"))
        legs = [Leg(f"host_w{w}", BeatmapDataModule(num_workers=w, **data)) for w in WORKERS]
        rec["resident_val_store"] = {}
        for b in BUDGETS:
            dm = ResidentBeatmapDataModule(num_workers=0, device=dev, resident_val=True, val_frame_budget=b,
                                           val_pad_multiple=2 * module.latent.chunk_size, **data)
            t0 = time.perf_counter()
            feed = dm.val_dataloader()
            torch.cuda.synchronize()
            rec["resident_val_store"][f"resident_{b}"] = {
                "bytes": feed.store.nbytes, "maps": len(feed.store), "build_s": round(time.perf_counter() - t0, 2), "groups": len(feed.groups),
                "maps_per_group": [len(g) for g in feed.groups], "padded_frames_share_per_group": [round(x, 4) for x in feed.padded_share()],
                "per_map_steps": len(feed.short)}
            legs.append(Leg(f"resident_{b}", dm))
        assert all(len(leg.dm.host.val_set.mapsets if hasattr(leg.dm, "host") else leg.dm.val_set.mapsets) == HELD_OUT for leg in legs)
        print(json.dumps(rec["resident_val_store"]), flush=True)
        for rep in range(args.reps + 1):                 # repetition 0: one untimed epoch each (first launches, workspaces, the page cache)
            for leg in legs:
                if leg.dead:
                    continue
                dt = leg.epoch(trainer, module, dev)
                if rep == 0:
                    leg.warm = dt
                else:
                    leg.runs.append(dt)
                print(json.dumps({"rep": rep, "leg": leg.name, "s": round(dt, 3)}), flush=True)
                if dt > args.leg_timeout:
                    leg.dead = f"an epoch took {dt:.1f} s, over the limit of {args.leg_timeout} s"
        out = {}
        for leg in legs:
            if not leg.runs:
                out[leg.name] = {"timed_out": leg.dead, "warm_up_epoch_s": round(leg.warm, 3)}
                continue
            out[leg.name] = {"epoch_s": [round(x, 3) for x in leg.runs], "epoch_s_median": round(statistics.median(leg.runs), 3),
                             "epoch_s_spread": round(max(leg.runs) - min(leg.runs), 3), "warm_up_epoch_s": round(leg.warm, 3),
                             "eval/score": leg.logs["eval/score"], "val/loss": leg.logs["val/loss"], **({"timed_out": leg.dead} if leg.dead else {})}
        rec["legs"] = out
        host = {n: v for n, v in out.items() if n.startswith("host_") and "epoch_s_median" in v}
        if host:
            best = min(host, key=lambda n: host[n]["epoch_s_median"])
            rec["parent_leg"] = best
            rec["resident_over_parent"] = {
                n: {"speedup": round(host[best]["epoch_s_median"] / v["epoch_s_median"], 3),
                    "gain_s": round(host[best]["epoch_s_median"] - v["epoch_s_median"], 3),
                    "beats_parent_spread": host[best]["epoch_s_median"] - v["epoch_s_median"] > host[best]["epoch_s_spread"]}
                for n, v in out.items() if n.startswith("resident_") and "epoch_s_median" in v}
        del legs
    rec["calibration_after"] = calibration(dev)
    line = json.dumps(rec)
    print(line, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "a") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
