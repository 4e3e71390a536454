"""What one validation check of `fit-denoiser` costs, per map from the host loader and in groups from a resident store
(`data.resident_val`, osu_dreamer_amd/resident.py: ResidentLatentValFeed; train.py: DiffusionTrainer._validation_group).

Whole validation epochs — fit.Trainer.validate on the DiffusionTrainer of the shipped model.yml, bf16-mixed — over 256 held-out maps of
300 .. 1500 latent frames written by write_synthetic_dataset, the feed included.  Legs, on one trainer (validation changes no state):

  host_w0         LatentDataModule.val_dataloader(), num_workers 0: the maps are read in the trainer's process
  host_w13        the same, data.num_workers 13 as shipped (validation then reads through ONE worker process)
  resident_<b>    ResidentLatentDataModule(resident_val=True, val_frame_budget=b): a quarter of, once and twice the default budget

A host leg builds its DataLoader anew every epoch, as fit.Trainer.validate does; the resident legs build their store once, before the
first (untimed) epoch, and its build time is reported apart.  Method (tools/mb_latent_val.py's): the legs alternate within each
repetition in one process, one untimed epoch each first, medians and spreads (max - min) of `--reps` epochs, host clocks around an epoch
that ends in a device synchronise, a bare-MFMA calibration before and after, the library's source hash.  Every resident leg reports the
share of padded frames of each of its groups.  Last, one epoch of host_w0 and one of the default-budget resident leg with every map's
t and x0 pinned to the same values: their val/* differ by the two paths' arithmetic only.

  python tools/mb_denoiser_val.py [--reps 5] [--out profiles/r19_denoiser_val.txt]
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
from osu_dreamer_amd.data import LatentDataModule, RaggedLatentValBatch, write_synthetic_dataset  # noqa: E402
from osu_dreamer_amd.fit import DEFAULT_CONFIG, build_from_config  # noqa: E402
from osu_dreamer_amd.resident import DEFAULT_VAL_FRAME_BUDGET, ResidentLatentDataModule  # noqa: E402
from tools.mb_bucketed_train import calibration  # noqa: E402

WORKERS = (0, 13)             # fixed: never sized by the machine's CPU count
HELD_OUT, TRAIN = 256, 4      # one map per mapset; the training maps only let the data modules be built
BUDGETS = (DEFAULT_VAL_FRAME_BUDGET // 4, DEFAULT_VAL_FRAME_BUDGET, DEFAULT_VAL_FRAME_BUDGET * 2)
LO, HI = 300, 1500


def lengths_of(n):
    """`n` lengths spread evenly over 300 .. 1500 latent frames, in a scrambled (seeded) order."""
    lens = [LO + round(i * (HI - LO) / max(n - 1, 1)) for i in range(n)]
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


def pinned_epoch(trainer, module, dm, lens, dev):
    """One validation epoch with map m's draws pinned to a generator seeded by m, whichever loader hands the map over."""
    vb, E = module.val_batches, module.diffusion.emb_dim
    step = type(module).validation_step

    def draw(m, width):
        gen = torch.Generator().manual_seed(1000 + m)
        t = torch.rand(vb, generator=gen) * 0.9 + 0.05
        x0 = torch.randn(vb, E, HI // vb + 1, generator=gen)[..., :lens[m] // vb]
        return t.to(dev), torch.nn.functional.pad(x0, (0, width - x0.shape[-1])).to(dev)

    def validation_step(batch, batch_idx):
        if isinstance(batch, RaggedLatentValBatch):
            pairs = [draw(m, batch.z.shape[-1]) for m in dm.val_feed.groups[batch_idx].tolist()]
            return step(module, batch, batch_idx, t=torch.cat([p[0] for p in pairs]), x0=torch.cat([p[1] for p in pairs]))
        t, x0 = draw(batch_idx, lens[batch_idx] // vb)
        return step(module, batch, batch_idx, t=t, x0=x0)
    module.validation_step = validation_step
    try:
        return trainer.validate(module, dm, dev)
    finally:
        del module.validation_step


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--leg-timeout", type=float, default=60.0, help="a leg whose epoch took longer leaves the rotation")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r19_denoiser_val.txt"), help="the record is appended to this file")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("mb_denoiser_val measures on an MI355X: no GPU is visible")
    _lib.lib()
    dev = torch.device("cuda:0")
    rec = {"tool": "mb_denoiser_val", "kernel_src_sha": _lib.source_sha(), "device": torch.cuda.get_device_name(0), "dtype": "bf16-mixed",
           "model": "model.yml defaults", "reps": args.reps,
           "what": "whole validation epochs (fit.Trainer.validate) over the held-out maps, feed included",
           "calibration_before": calibration(dev)}
    with tempfile.TemporaryDirectory() as tmp:
        t0 = time.perf_counter()
        lens = lengths_of(HELD_OUT) + [LO] * TRAIN             # the hold-out rule takes the first mapsets of the sorted listing
        cfg = yaml.safe_load(open(DEFAULT_CONFIG))
        m = cfg["model"]
        write_synthetic_dataset(os.path.join(tmp, "data"), n_maps=len(lens), frames=lens, a_dim=m["a_dim"], emb_dim=m["emb_dim"],
                                style_dim=m["style_dim"], seed=2)
        rec["dataset"] = {"held_out_maps": HELD_OUT, "lengths": f"{LO} .. {HI} latent frames, evenly spread, scrambled",
                          "frames": sum(lens[:HELD_OUT]), "write_s": round(time.perf_counter() - t0, 1)}
        print(json.dumps(rec["dataset"]), flush=True)
        cfg["trainer"].update(default_root_dir=tmp, enable_checkpointing=False)
        torch.manual_seed(0)
        module, trainer = build_from_config(cfg)
        module.to(dev)
        rec["val_batches"] = module.val_batches
        data = {k: v for k, v in cfg["data"].items() if k not in ("num_workers", "resident", "resident_max_gb", "resident_val", "val_frame_budget")}
        data.update(max_val_count=HELD_OUT, max_val_frac=0.99, data_path=os.path.join(tmp, "data"))
        legs = [Leg(f"host_w{w}", LatentDataModule(num_workers=w, **data)) for w in WORKERS]
        rec["resident_val_store"] = {}
        for b in BUDGETS:
            dm = ResidentLatentDataModule(num_workers=0, device=dev, resident_val=True, val_frame_budget=b, val_batches=module.val_batches, **data)
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
                             "val/loss (own draws)": leg.logs["val/loss"], **({"timed_out": leg.dead} if leg.dead else {})}
        rec["legs"] = out
        host = {n: v for n, v in out.items() if n.startswith("host_") and "epoch_s_median" in v}
        if host:
            best = min(host, key=lambda n: host[n]["epoch_s_median"])
            rec["parent_leg"] = best
            rec["resident_over_parent"] = {
                n: {"speedup": round(host[best]["epoch_s_median"] / v["epoch_s_median"], 3),
                    "gain_s": round(host[best]["epoch_s_median"] - v["epoch_s_median"], 3),
                    "gain_over_parent_spread": (round((host[best]["epoch_s_median"] - v["epoch_s_median"]) / host[best]["epoch_s_spread"], 1)
                                                if host[best]["epoch_s_spread"] > 0 else None)}
                for n, v in out.items() if n.startswith("resident_") and "epoch_s_median" in v}
        rec["pinned_draws"] = {leg.name: pinned_epoch(trainer, module, leg.dm, lens, dev)
                               for leg in legs if leg.name in ("host_w0", f"resident_{DEFAULT_VAL_FRAME_BUDGET}")}
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
