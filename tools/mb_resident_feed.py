"""How much of a real training epoch waits for the host loader, and what the device-resident feed (osu_dreamer_amd/resident.py) does to it.

Whole epochs, LOADER INCLUDED, of full training steps (zero_grad, forward, backward, clip + AdamW + EMA — fit.Trainer.train_group) on a
write_synthetic_dataset tree, three cases:

  windows    fit-denoiser on fixed windows, the reference's own shape: batch 128 x 152 frames, max_per_map 1 (model.yml)
  bucketed   fit-denoiser on frame-budget whole maps: batch_frames 11280, bucket_pool 128, the map lengths of profiles/r13_bucketed_train.txt
  style      fit-style at batch 512 (style.yml: seq_len 1, max_per_map 1)

Each case runs four legs on trainers of their own holding the same weights: the host loader (LatentDataModule) with num_workers 0, 8 and 16,
and the resident feed.  A loader leg builds its DataLoader anew every epoch, as fit.Trainer does.  Method (tools/mb_bucketed_train.py's):
the legs alternate within each repetition in one process, one untimed epoch each first, medians of `--reps` epochs, host clocks around an
epoch that ends in a device synchronise, a bare-MFMA calibration before and after, the library's source hash.  Every leg's epoch runs under
a time limit of its own (`--leg-timeout` seconds, checked after every step): a leg that exceeds it is reported as timed out and leaves the
rotation.

Per leg the record also carries `outside_steps_fraction`: the share of the epoch's wall time that lies outside every step's span on the
stream (an event recorded when the batch has reached the device, one after the step's last launch).  When the host runs ahead the spans
tile the timeline and the share is ~0; when the device waits for the next batch it is that wait — the time the device had no kernel of a
step running (the resident leg's gather kernels and the loader legs' host-to-device copies fall into it too, so it bounds the idle time
from above).  The resident legs add od_feed_gather's own time per batch.

The windows and style cases train on `--maps` maps (default 8192): the loader batches inside each worker, over that worker's shard of the
files, and drops the partial batch, so with 16 workers and batch 512 a smaller set yields no batch at all from those legs.

  python tools/mb_resident_feed.py [--maps 8192] [--reps 5] [--out profiles/r14_resident_feed.txt]
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

from oracle import denoiser_oracle as O  # noqa: E402
from osu_dreamer_amd import _lib, ops  # noqa: E402
from osu_dreamer_amd.data import LatentDataModule, write_synthetic_dataset  # noqa: E402
from osu_dreamer_amd.fit import DEFAULT_STYLE_CONFIG, Trainer, build_style_from_config  # noqa: E402
from osu_dreamer_amd.resident import STYLE_FIELDS, ResidentLatentDataModule  # noqa: E402
from tools.mb_bucketed_train import HELD_OUT, calibration, lengths_of, make_trainer  # noqa: E402

WORKERS = (0, 8, 16)          # never more than 16 loader processes beside the trainer
CASES = {
    "windows": dict(batch_size=128, seq_len=152, max_per_map=1, shuffle_buffer_size=512),
    "bucketed": dict(batch_size=64, seq_len=None, max_len=1536, pad_multiple=64, batch_frames=11280, bucket_pool=128),
    "style": dict(batch_size=512, seq_len=1, max_per_map=1, shuffle_buffer_size=512),
}


class LegTimeout(Exception):
    pass


class Leg:
    def __init__(self, case, name, dm, module, opt, sched, trainer, dev, limit):
        self.case, self.name, self.dm, self.dev, self.limit = case, name, dm, dev, limit
        self.module, self.opt, self.sched, self.trainer = module, opt, sched, trainer
        self.times, self.outside, self.units, self.steps, self.dead = [], [], 0, 0, None

    def epoch(self):
        """One epoch, loader included: (seconds, seconds inside the steps' spans, samples or valid frames, steps)."""
        loader = self.dm.train_dataloader()
        spans, units, i = [], 0, 0
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        it = iter(loader)
        while True:
            batch = next(it, None)
            if batch is None:
                break
            batch = self.trainer._to(batch, self.dev)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            self.trainer.train_group(self.module, self.opt, self.sched, [batch], self.dev, i)
            e1.record()
            spans.append((e0, e1))
            units += int(batch.lengths.sum()) if len(batch) == 5 else int(batch[2].shape[0])
            i += 1
            if time.perf_counter() - t0 > self.limit:
                del it, loader
                raise LegTimeout(f"{self.case}/{self.name}: an epoch passed {self.limit} s at step {i}")
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        del it, loader                           # a loader leg's workers end here: at most 16 are alive at a time
        return dt, sum(a.elapsed_time(b) for a, b in spans) * 1e-3, units, i


def denoiser_legs(case, data_path, d, P, dev, root, limit):
    legs = []
    common = dict(max_val_count=HELD_OUT, max_val_frac=.3, data_path=data_path, **CASES[case])
    for name, dm in [(f"loader_w{w}", LatentDataModule(num_workers=w, **common)) for w in WORKERS] + \
                    [("resident", ResidentLatentDataModule(num_workers=0, device=dev, **common))]:
        module, opt, sched = make_trainer(d, P, dev)
        legs.append(Leg(case, name, dm, module, opt, sched, Trainer(precision="bf16-mixed", default_root_dir=root, enable_checkpointing=False), dev, limit))
    return legs


def style_legs(data_path, dev, root, limit):
    cfg = yaml.safe_load(open(DEFAULT_STYLE_CONFIG))
    cfg["trainer"].update(default_root_dir=root, enable_checkpointing=False)
    legs = []
    common = dict(max_val_count=HELD_OUT, max_val_frac=.3, data_path=data_path, **CASES["style"])
    state = None
    for name, dm in [(f"loader_w{w}", LatentDataModule(num_workers=w, **common)) for w in WORKERS] + \
                    [("resident", ResidentLatentDataModule(num_workers=0, device=dev, fields=STYLE_FIELDS, **common))]:
        module, trainer = build_style_from_config(cfg)
        state = state or {k: v.clone() for k, v in module.state_dict().items()}
        module.load_state_dict(state)
        module.gradient_clip_val = trainer.gradient_clip_val
        module.to(dev)
        oc = module.configure_optimizers()
        legs.append(Leg("style", name, dm, module, oc["optimizer"], oc["lr_scheduler"]["scheduler"], trainer, dev, limit))
    return legs


def gather_times(leg, dev):
    """od_feed_gather on the resident leg's own batches: the whole gather of a batch (descriptor copy, the two kernels, the two
    index_selects) as a device span over one planned epoch, and the h kernel alone, back to back, on the epoch's first batch."""
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
    out = {"batches": len(plan), "gather_us_per_batch_device_span": round(e0.elapsed_time(e1) * 1e3 / len(plan), 1),
           "gather_us_per_batch_host_launch": round(host * 1e6 / len(plan), 1)}
    st = leg.dm.store
    if st.has_frames:
        pb = plan[0]
        B = len(pb.maps)
        base = torch.from_numpy(st.h_base[pb.maps] + pb.starts).to(dev)
        cs = torch.from_numpy(st.h_stride[pb.maps]).to(dev)
        lens = torch.from_numpy(pb.lens).to(torch.int32).to(dev)
        h = torch.empty(B, st.a_dim, pb.Lpad, device=dev)
        ops.feed_gather(st.data, base, cs, lens, h)
        torch.cuda.synchronize()
        e0.record()
        for _ in range(20):
            ops.feed_gather(st.data, base, cs, lens, h)
        e1.record()
        torch.cuda.synchronize()
        us = e0.elapsed_time(e1) * 1e3 / 20
        moved = 4 * (int(pb.lens.sum()) * st.a_dim + h.numel())               # bytes read + bytes written
        out.update(h_kernel_us=round(us, 1), h_shape=list(h.shape), h_kernel_GBps=round(moved / us * 1e-3, 1),
                   note="20 launches on one batch, back to back: the source stays in the caches, so this is the kernel's rate, not HBM's")
    return out


def run_case(case, legs, reps, unit):
    for leg in legs:                                 # one untimed epoch each: first launches, workspaces, the page cache
        try:
            leg.warm = leg.epoch()[0]
        except LegTimeout as e:
            leg.dead = str(e)
    for _ in range(reps):
        for leg in legs:
            if leg.dead:
                continue
            try:
                dt, inside, units, steps = leg.epoch()
            except LegTimeout as e:
                leg.dead = str(e)
                continue
            leg.times.append(dt)
            leg.outside.append(1.0 - inside / dt)
            leg.units, leg.steps = units, steps
    out = {}
    for leg in legs:
        if leg.dead or not leg.times:
            out[leg.name] = {"timed_out": leg.dead}
            continue
        med = statistics.median(leg.times)
        out[leg.name] = {"epoch_s": [round(t, 4) for t in leg.times], "epoch_s_median": round(med, 4), "warm_up_epoch_s": round(leg.warm, 3),
                         "steps": leg.steps, unit: leg.units, f"{unit}_per_s": round(leg.units / med, 1),
                         "ms_per_step_median": round(med / max(leg.steps, 1) * 1e3, 2),
                         "outside_steps_fraction": round(statistics.median(leg.outside), 4)}
    res = out.get("resident", {}).get(f"{unit}_per_s")
    alive = {n: v[f"{unit}_per_s"] for n, v in out.items() if n != "resident" and f"{unit}_per_s" in v}
    if res and alive:
        best = max(alive, key=alive.get)
        out["resident_over_best_loader"] = {"best_loader": best, "ratio": round(res / alive[best], 3)}
        out["loader_keeps_up"] = {n: bool(v >= 0.97 * res) for n, v in alive.items()}       # within 3 % of the resident feed's rate
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--maps", type=int, default=8192, help="training maps of the windows and style cases (the bucketed case: 256, as profiles/r13)")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--depth", type=int, default=8)
    ap.add_argument("--leg-timeout", type=float, default=120.0, help="seconds one epoch of one leg may take")
    ap.add_argument("--cases", default="windows,bucketed,style")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r14_resident_feed.txt"), help="the record is appended to this file")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("mb_resident_feed measures on an MI355X: no GPU is visible")
    _lib.lib()
    dev = torch.device("cuda:0")
    d = O.Dims(depth=args.depth)
    P = O.init_params(d, seed=1)
    rec = {"tool": "mb_resident_feed", "kernel_src_sha": _lib.source_sha(), "device": torch.cuda.get_device_name(0), "dtype": "bf16",
           "model": f"model.yml defaults, depth {d.depth}; style.yml defaults", "reps": args.reps, "loader_workers": list(WORKERS),
           "what": "whole epochs of full training steps, loader included; a loader leg builds its DataLoader every epoch, as fit.Trainer does",
           "calibration_before": calibration(dev), "cases": {}}
    with tempfile.TemporaryDirectory() as tmp:
        big, small = os.path.join(tmp, "big"), os.path.join(tmp, "r13")
        t0 = time.perf_counter()
        write_synthetic_dataset(big, n_maps=args.maps + HELD_OUT, frames=lengths_of(args.maps + HELD_OUT), a_dim=d.a_dim, emb_dim=d.emb_dim,
                                style_dim=d.style_dim, seed=2)
        write_synthetic_dataset(small, n_maps=256 + HELD_OUT, frames=lengths_of(256 + HELD_OUT), a_dim=d.a_dim, emb_dim=d.emb_dim,
                                style_dim=d.style_dim, seed=2)
        rec["dataset"] = {"windows_and_style_maps": args.maps, "bucketed_maps": 256, "lengths": "300 .. 1500, evenly spread, scrambled; one map per mapset",
                          "write_s": round(time.perf_counter() - t0, 1)}
        for case in args.cases.split(","):
            torch.manual_seed(0)
            t0 = time.perf_counter()
            if case == "style":
                legs, unit = style_legs(big, dev, tmp, args.leg_timeout), "samples"
            else:
                legs = denoiser_legs(case, big if case == "windows" else small, d, P, dev, tmp, args.leg_timeout)
                unit = "samples" if case == "windows" else "valid_frames"
            out = run_case(case, legs, args.reps, unit)
            res = legs[-1]
            out["resident_store"] = {"bytes": res.dm.store.nbytes, "maps": len(res.dm.store), "build_s_included_in_case_s": True}
            out["od_feed_gather"] = gather_times(res, dev)
            out["data_args"] = {k: v for k, v in CASES[case].items()}
            out["case_s"] = round(time.perf_counter() - t0, 1)
            rec["cases"][case] = out
            print(json.dumps({case: out}), flush=True)
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
