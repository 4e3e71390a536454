"""What a ragged training step costs: one step (forward + backward, no optimizer pass) of the default denoiser (model.yml: depth 8, D = 512,
16 heads of 64; 46.9 M parameters) in bf16 on B = 8 songs of 300 .. 1500 latent frames padded to Lpad = 1536, three ways in one process:

  ragged        DiffusionTrainer.forward(..., lengths=): the varlen kernels, every song at its own length
  padded_dense  the same (B, Lpad) tensors without lengths — the dense step as it was before ragged training existed: the cost of
                training on the padding (and the wrong loss: padded frames count)
  single_sum    the B songs one after the other as dense B = 1 steps at L = lengths[b]

Every leg, and every song of single_sum, runs on a DiffusionTrainer of its own holding the same weights, so no timed call re-plans the
engine's workspace or re-allocates anything: the figures are kernel and launch time.  (One model looping over whole maps of changing
length, as a dense whole-map run does today, would also pay a workspace allocation per step; that is not counted here.)

The legs alternate within each repetition; times are host clocks around work that ends in a device synchronise, after a warm-up of every
leg.  The record carries the library's source hash and a bare-MFMA calibration of the box (bench.mfma_calibration) taken before and after.
Expectation to report against: ragged <= padded_dense and ragged < single_sum.

  python tools/mb_ragged_train.py [--reps 7] [--out profiles/r12_ragged_train.txt]
"""
import argparse
import json
import os
import statistics
import sys
import time

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=7)
ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "r12_ragged_train.txt"),
                help="the record is appended to this file")
ap.add_argument("--depth", type=int, default=8)
args = ap.parse_args()
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from oracle import denoiser_oracle as O  # noqa: E402
from osu_dreamer_amd import _lib  # noqa: E402
from osu_dreamer_amd.lr_schedule import LRScheduleArgs  # noqa: E402
from osu_dreamer_amd.model import BackboneArgs, DiffusionModelArgs  # noqa: E402
from osu_dreamer_amd.train import DiffusionTrainer  # noqa: E402

if not torch.cuda.is_available():
    raise SystemExit("mb_ragged_train measures on an MI355X: no GPU is visible")
dev = torch.device("cuda:0")
_lib.lib()
B, LPAD = 8, 1536
LENS = [300 + round(i * 1200 / (B - 1)) for i in range(B)]          # 300 .. 1500, evenly spread
d = O.Dims(depth=args.depth)
P = O.init_params(d, seed=1)


def make():
    tr = DiffusionTrainer(val_batches=2, opt_args=dict(lr=3e-4, weight_decay=0.01),
                          schedule_args=LRScheduleArgs(warmup_init=.3, warmup_steps=1000, decay_start=30000),
                          osl_weight=1., del_weight=30., emb_dim=d.emb_dim, a_dim=d.a_dim, style_dim=d.style_dim,
                          diffusion_args=DiffusionModelArgs(d.global_cond_dim, d.backbone_dim,
                                                            BackboneArgs(d.depth, d.expand, d.head_dim, d.n_heads, d.radius), d.u_head_dim))
    tr.diffusion.load_state_dict(P)
    tr = tr.to(dev)
    tr.diffusion.compute_dtype = torch.bfloat16
    return tr, tr.configure_optimizers()["optimizer"]


data = {k: v.to(dev) for k, v in O.synthetic_batch(d, B, LPAD, seed=2).items()}
for b, n in enumerate(LENS):
    for k in ("h", "z", "x0"):
        data[k][b, :, n:] = 0
singles = [{k: (v[b:b + 1, :, :n] if v.dim() == 3 else v[b:b + 1]).contiguous() for k, v in data.items()} for b, n in enumerate(LENS)]
tr_r, opt_r = make()
tr_p, opt_p = make()
tr_s = [make() for _ in LENS]


def one(tr, dd, lengths=None):
    loss, _ = tr(tr.diffusion, dd["h"], dd["z"], dd["s"], None, lengths=lengths, t=dd["t"], x0=dd["x0"])
    loss.backward()
    return loss


def ragged():
    opt_r.zero_grad()
    return float(one(tr_r, data, LENS).detach())


def padded_dense():
    opt_p.zero_grad()
    return float(one(tr_p, data).detach())


def single_sum():
    total = 0.0
    for (tr, opt), s in zip(tr_s, singles):
        opt.zero_grad()
        total += float(one(tr, s).detach())
    return total / B


def timed(fn):
    torch.cuda.synchronize()
    t = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t


def calibration():
    try:
        import bench
        return bench.mfma_calibration(dev)
    except Exception as e:          # the record says so rather than carrying no calibration silently
        return {"error": repr(e)}


LEGS = (("ragged", ragged), ("padded_dense", padded_dense), ("single_sum", single_sum))
cal0 = calibration()
losses = {n: f() for n, f in LEGS}                                   # warm-up of every leg (and every single-song plan)
for _, f in LEGS:
    f()
times = {n: [] for n, _ in LEGS}
for _ in range(args.reps):
    for n, f in LEGS:
        times[n].append(timed(f))
cal1 = calibration()
med = {n: statistics.median(v) for n, v in times.items()}
rec = {"tool": "mb_ragged_train", "kernel_src_sha": _lib.source_sha(), "device": torch.cuda.get_device_name(0), "dtype": "bf16",
       "model": f"model.yml defaults, depth {d.depth}", "B": B, "Lpad": LPAD, "lengths": LENS, "valid_frames": sum(LENS),
       "padded_frames": B * LPAD, "what": "forward + backward of one training step, no optimizer pass; ms",
       "ms": {n: [round(t * 1e3, 2) for t in v] for n, v in times.items()},
       "ms_median": {n: round(t * 1e3, 2) for n, t in med.items()},
       "ragged_over_padded_dense": round(med["ragged"] / med["padded_dense"], 3),
       "ragged_over_single_sum": round(med["ragged"] / med["single_sum"], 3),
       "expectation_ragged_le_padded_dense": bool(med["ragged"] <= med["padded_dense"]),
       "expectation_ragged_lt_single_sum": bool(med["ragged"] < med["single_sum"]),
       "attention_backward": {"ragged": "pair" if not tr_r.diffusion.engine.fused_attn_bwd() else "fused",
                              "padded_dense": "fused" if tr_p.diffusion.engine.fused_attn_bwd() else "pair"},
       "loss": {n: round(v, 5) for n, v in losses.items()},
       "loss_note": "ragged and single_sum are the same quantity; padded_dense also averages over the padded frames",
       "calibration_before": cal0, "calibration_after": cal1}
line = json.dumps(rec)
print(line, flush=True)
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "a") as f:
        f.write(line + "\n")
