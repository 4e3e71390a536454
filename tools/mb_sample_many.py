"""What batching songs into one sampler call gains: a Python loop of DiffusionModel.sample() calls (one per song) against one
DiffusionModel.sample_many call, for G songs of 2-4 minutes (latent L_g in 750..1500) with 4 difficulties each, at 8 and 50 steps, in the
three precision modes.  Device-synchronised wall time after a warm-up call of each form; the two forms alternate within one process.
Prints one JSON line per (mode, steps, G) with latent frames per second (sum of B_g * L_g per call / seconds) and the library's source hash.

  python tools/mb_sample_many.py [--reps 3] [--gs 1,2,4,8] [--steps 8,50] [--modes fp32,fp32_bf16x3,bf16]
  python tools/mb_sample_many.py --single [--root DIR]     # single-song sample() at configs[3] (B = 4, L = 1115, 50 steps) only:
                                                           # run it against another tree's package + library (--root) for an A/B
"""
import argparse
import json
import os
import statistics
import sys
import time

ap = argparse.ArgumentParser()
ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))), help="tree whose package and library run")
ap.add_argument("--single", action="store_true")
ap.add_argument("--reps", type=int, default=3)
ap.add_argument("--gs", default="1,2,4,8")
ap.add_argument("--steps", default="8,50")
ap.add_argument("--tag", default="")
ap.add_argument("--modes", default="fp32,fp32_bf16x3,bf16")
args = ap.parse_args()
sys.path.insert(0, args.root)

import torch  # noqa: E402

from oracle import denoiser_oracle as O  # noqa: E402
from osu_dreamer_amd import _lib  # noqa: E402
from osu_dreamer_amd.model import BackboneArgs, DiffusionModel, DiffusionModelArgs  # noqa: E402

MODES = (("fp32", None, "f32"), ("fp32_bf16x3", None, "bf16x3"), ("bf16", torch.bfloat16, "f32"))
dev = torch.device("cuda:0")
_lib.lib()
sha = _lib.source_sha()
d = O.Dims(depth=8)
m = DiffusionModel(d.emb_dim, d.a_dim, d.style_dim, DiffusionModelArgs(d.global_cond_dim, d.backbone_dim,
                   BackboneArgs(d.depth, d.expand, d.head_dim, d.n_heads, d.radius), d.u_head_dim))
m.load_state_dict(O.init_params(d, seed=1))
m = m.to(dev).eval()


def timed(fn):
    torch.cuda.synchronize()
    t = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t


def song(L, B, seed):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(1, d.a_dim, L, generator=g).to(dev), torch.randn(B, d.style_dim, generator=g).to(dev),
            torch.randn(B, d.emb_dim, L, generator=g).to(dev))


if args.single:
    a, s, x = song(1115, 4, 0)
    for mode, dt, mm in MODES:
        m.compute_dtype, m.f32_matmul = dt, mm
        with torch.no_grad():
            m.sample(a, s, 50, x_init=x)
            ts = [timed(lambda: m.sample(a, s, 50, x_init=x)) for _ in range(args.reps)]
        print(json.dumps({"tool": "mb_sample_many --single", "tag": args.tag, "kernel_src_sha": sha, "mode": mode, "B": 4, "L": 1115,
                          "steps": 50, "ms": [round(t * 1e3, 2) for t in ts], "ms_median": round(statistics.median(ts) * 1e3, 2)}),
              flush=True)
    sys.exit(0)

gen = torch.Generator().manual_seed(5)
lengths = [int(x) for x in torch.randint(750, 1501, (8,), generator=gen)]
songs = [song(L, 4, 10 + i) for i, L in enumerate(lengths)]
for mode, dt, mm in MODES:
    if mode not in args.modes.split(","):
        continue
    m.compute_dtype, m.f32_matmul = dt, mm
    for steps in [int(x) for x in args.steps.split(",")]:
        for G in [int(x) for x in args.gs.split(",")]:
            sg = songs[:G]
            frames = sum(s[1].shape[0] * s[0].shape[-1] for s in sg)

            def loop():
                for a, s, x in sg:
                    m.sample(a, s, steps, x_init=x)

            def batched():
                m.sample_many([x[0] for x in sg], [x[1] for x in sg], steps, x_init=[x[2] for x in sg])

            with torch.no_grad():
                loop()
                batched()
                tl, tb = [], []
                for _ in range(args.reps):
                    tl.append(timed(loop))
                    tb.append(timed(batched))
            ml, mb = statistics.median(tl), statistics.median(tb)
            print(json.dumps({"tool": "mb_sample_many", "kernel_src_sha": sha, "mode": mode, "steps": steps, "G": G, "B": 4 * G,
                              "lengths": [x[0].shape[-1] for x in sg], "Lpad": (max(x[0].shape[-1] for x in sg) + 63) // 64 * 64,
                              "loop_ms": round(ml * 1e3, 2), "batched_ms": round(mb * 1e3, 2),
                              "loop_frames_per_s": round(frames / ml), "batched_frames_per_s": round(frames / mb),
                              "speedup": round(ml / mb, 3)}), flush=True)
