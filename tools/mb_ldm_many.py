"""What batching the non-denoiser stages gains: LDM.sample_many as it stands (one audio-encoder call, one style-sampler call, the batched
denoiser sampler, then LDM._decode_songs: one varlen decoder call in bf16, per-song decoder calls in fp32) against the per-song-stage form it replaced (audio encoder, style sampler and decoder in a
Python loop over the songs around the same batched denoiser call), for G songs of 2-4 minutes with 4 difficulties each, at 8 and 50
steps, in the three precision modes, with bench.py's ldm_sample model (default widths).  Per-stage times from HIP events on the launch
stream; the two forms alternate within one process after a warm-up call of each.  Then `encode-latents` throughput on a generated
64-map dataset: one map (and one mapset's audio) per call against the default frame budget.  One JSON line per measurement, with the
library's source hash.

  python tools/mb_ldm_many.py [--reps 2] [--gs 1,2,4,8] [--steps 8,50] [--modes fp32,fp32_bf16x3,bf16] [--no-encode]
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
ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=2)
ap.add_argument("--gs", default="1,2,4,8")
ap.add_argument("--steps", default="8,50")
ap.add_argument("--modes", default="fp32,fp32_bf16x3,bf16")
ap.add_argument("--no-encode", action="store_true")
args = ap.parse_args()

import numpy as np  # noqa: E402
import torch  # noqa: E402

from bench import default_model_args  # noqa: E402
from osu_dreamer_amd import _lib  # noqa: E402
from osu_dreamer_amd.ldm import LDM, pad_to_multiple  # noqa: E402

MODES = (("fp32", None, "f32"), ("fp32_bf16x3", None, "bf16x3"), ("bf16", torch.bfloat16, "f32"))
STAGES = ("audio_encoder", "style_sampler", "denoiser_sampler", "decode")
dev = torch.device("cuda:0")
_lib.lib()
sha = _lib.source_sha()
torch.manual_seed(7)
m = LDM(dict(emb_dim=6, style_dim=32, n_downs=3, stride=3,
             latent_args=dict(h_dim=128, ae_args=dict(n_layers=8, expand=4, radius=2), style_head_dim=64, style_heads=16),
             style_args=dict(label_features=128, h_dim=256, depth=8, expand=4),
             diffusion_args=default_model_args()["diffusion_args"]))
g = torch.Generator().manual_seed(7)
with torch.no_grad():
    for n, p in m.named_parameters():
        if float(p.abs().max()) == 0.0:
            p.copy_(0.02 * torch.randn(p.shape, generator=g))
m = m.to(dev).eval()
c = m.latent.chunk_size
gen = torch.Generator().manual_seed(5)
lengths = [int(x) for x in torch.randint(20062, 40125, (8,), generator=gen)]       # 2-4 minutes at bench.py's 30093 frames / 3 min
songs = [(torch.randn(72, L, generator=gen).to(dev), (torch.rand(4, 5, generator=gen) * 10).to(dev)) for L in lengths]


def per_song_stages(sg, steps, ev):
    """The per-song-stage form (LDM.sample_many before the latent kernels had varlen forms)."""
    enc = []
    ev[0].record()
    for a, _ in sg:
        enc.append(m.latent.audio_encoder(pad_to_multiple(a, c)[None]))
    ev[1].record()
    ss = [m.style.sample(lab) for _, lab in sg]
    ev[2].record()
    zs = m.diffusion.sample_many([e[1] for e in enc], ss, steps)
    ev[3].record()
    out = [m.latent.decode(z, s, skips=e[0]) for z, s, e in zip(zs, ss, enc)]
    ev[4].record()
    return out


def batched_stages(sg, steps, ev):
    """LDM.sample_many's body, with events between its stages."""
    Ls = [a.shape[-1] for a, _ in sg]
    Lps = [-(-L // c) * c for L in Ls]
    ev[0].record()
    audio = torch.zeros(len(sg), 72, max(Lps), device=dev)
    for i, (a, _) in enumerate(sg):
        audio[i, :, :Lps[i]] = pad_to_multiple(a, c)
    skips, h = m.latent.audio_encoder(audio, lengths=Lps)
    ev[1].record()
    ss = m.style.sample_many([lab for _, lab in sg])
    ev[2].record()
    zs = m.diffusion.sample_many([h[i:i + 1, :, :Lps[i] // c] for i in range(len(sg))], ss, steps)
    ev[3].record()
    out = m._decode_songs(zs, ss, skips, Lps)
    ev[4].record()
    return out


def timed(fn, sg, steps):
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(5)]
    torch.cuda.synchronize()
    t = time.perf_counter()
    fn(sg, steps, ev)
    torch.cuda.synchronize()
    wall = (time.perf_counter() - t) * 1e3
    return wall, [ev[i].elapsed_time(ev[i + 1]) for i in range(4)]


def med(xs):
    return round(statistics.median(xs), 2)


for mode, dt, mm in MODES:
    if mode not in args.modes.split(","):
        continue
    m.set_precision(dt, mm)
    for steps in [int(x) for x in args.steps.split(",")]:
        for G in [int(x) for x in args.gs.split(",")]:
            sg = songs[:G]
            with torch.no_grad():
                timed(per_song_stages, sg, steps)
                timed(batched_stages, sg, steps)
                rl, rb = [], []
                for _ in range(args.reps):
                    rl.append(timed(per_song_stages, sg, steps))
                    rb.append(timed(batched_stages, sg, steps))
            line = {"tool": "mb_ldm_many", "kernel_src_sha": sha, "mode": mode, "steps": steps, "G": G, "B": 4 * G,
                    "lengths": [a.shape[-1] for a, _ in sg],
                    "loop_wall_ms": med([r[0] for r in rl]), "batched_wall_ms": med([r[0] for r in rb])}
            for i, st in enumerate(STAGES):
                line[f"loop_{st}_ms"] = med([r[1][i] for r in rl])
                line[f"batched_{st}_ms"] = med([r[1][i] for r in rb])
            nd = [0, 1, 3]
            line["loop_non_denoiser_ms"] = round(sum(line[f"loop_{STAGES[i]}_ms"] for i in nd), 2)
            line["batched_non_denoiser_ms"] = round(sum(line[f"batched_{STAGES[i]}_ms"] for i in nd), 2)
            print(json.dumps(line), flush=True)

if not args.no_encode:
    from osu_dreamer_amd.encode_latents import encode_dataset
    from pathlib import Path
    rng = np.random.default_rng(0)
    lat = m.latent
    lat.compute_dtype, lat.f32_matmul = None, "f32"            # encode-latents' default precision
    with tempfile.TemporaryDirectory() as tmp:
        root = Path(tmp)
        for s in range(16):                                      # 16 mapsets x 4 maps, 1-3 minutes
            L = int(rng.integers(10031, 30094))
            d = root / f"{s:02d}"
            d.mkdir()
            np.save(d / "spec.npy", rng.integers(0, 256, (72, L), dtype=np.uint8))
            for k in range(4):
                with open(d / f"{k}.map.npy", "wb") as f:
                    np.savez(f, hit=rng.integers(0, 256, (7, L), dtype=np.uint8), xy=rng.integers(0, 65536, (2, L), dtype=np.uint16),
                             xy_min=np.zeros((2, 1)), xy_rng=np.full((2, 1), 512.0), labels=rng.uniform(0, 10, 5))
        with torch.no_grad():
            encode_dataset(lat, root, force=True, frame_budget=1)                # warm-up
            for name, budget in (("one_per_call", 1), ("batched", 1 << 19)):
                ts = []
                for _ in range(args.reps):
                    torch.cuda.synchronize()
                    t = time.perf_counter()
                    n, nh = encode_dataset(lat, root, force=True, frame_budget=budget)
                    torch.cuda.synchronize()
                    ts.append(time.perf_counter() - t)
                print(json.dumps({"tool": "mb_ldm_many encode-latents", "kernel_src_sha": sha, "form": name, "frame_budget": budget,
                                  "maps": n, "mapsets": nh, "s": [round(x, 3) for x in ts],
                                  "maps_per_s": round(n / statistics.median(ts), 2)}), flush=True)
