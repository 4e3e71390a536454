"""Attention at head_dim 128 against head_dim 64 at equal n_heads x head_dim (equal MFMA FLOPs, half the softmax rows), in one process:
HIP events, both sides warmed, the two sides alternating round by round, median per side.

    python tools/mb_attn_hd128.py [--rounds 7] [--iters 3] [--out record.json]
    OSU_DREAMER_HIP_LIB=path/to/variant.so python tools/mb_attn_hd128.py       (a variant built by tools/build_variant.sh)

  fwd_bf16_pre       B 32 x L 8192: 8 heads x 128 against 16 x 64, bf16, q pre-multiplied (what the training step launches)
  bwd_pair_bf16_pre  the same shape through ops.flash_attn_bwd (delta + dK/dV + dQ kernels)
  sampler_fwd_*      B 4 x L 1115 (the sampler's shape) forward in fp32, fp32-as-3-x-bf16 and bf16
The yardstick is what the SAME library dispatches for head_dim 64 in the same call.  Prints one line per comparison and a JSON record
(times in ms, ratio = head_dim 128 / head_dim 64, the library's source hash).
"""
import argparse
import json
import math
import os
import statistics
import sys

import torch

sys.path.insert(0, os.getcwd())
from osu_dreamer_amd import _lib, ops  # noqa: E402

DH = 1024                                  # n_heads x head_dim on both sides
SIDES = ((128, 8), (64, 16))               # (head_dim, n_heads)


def timed(fn, iters):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters


def compare(name, fns, rounds, iters, flops):
    """fns: {head_dim: callable}.  One warm-up call per side, then `rounds` rounds of (128, 64), each timing `iters` calls."""
    for fn in fns.values():
        fn()
    torch.cuda.synchronize()
    t = {hd: [] for hd in fns}
    for _ in range(rounds):
        for hd, fn in fns.items():
            t[hd].append(timed(fn, iters))
    med = {hd: statistics.median(v) for hd, v in t.items()}
    rec = {"name": name, "ms_hd128": med[128], "ms_hd64": med[64], "ratio_128_over_64": med[128] / med[64],
           "tflops_hd128": flops / med[128] / 1e9, "tflops_hd64": flops / med[64] / 1e9,
           "rounds_ms_hd128": t[128], "rounds_ms_hd64": t[64]}
    print(f"{name:20s} hd128 {med[128]:9.3f} ms ({rec['tflops_hd128']:6.1f} TF/s)   hd64 {med[64]:9.3f} ms ({rec['tflops_hd64']:6.1f} TF/s)   "
          f"ratio {rec['ratio_128_over_64']:.3f}", flush=True)
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=3)
    ap.add_argument("--out", default=None, help="also write the full record (every round's time) as JSON")
    a = ap.parse_args()
    _lib.lib()
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev).manual_seed(0)
    recs = []

    def problem(B, L, dtype, pre):
        M = B * L
        qk = torch.randn(M, 2 * DH, device=dev, generator=g)
        qkv = torch.randn(M, 3 * DH, device=dev, generator=g).to(dtype)
        return M, qk, qkv

    # ---- training shape, bf16, q pre-multiplied: forward and the two-kernel backward
    B, L, bf = 32, 8192, torch.bfloat16
    M, qk32, qkv = problem(B, L, bf, True)
    do = torch.randn(M, DH, device=dev, generator=g).to(bf)
    bufs = {}
    for hd, H in SIDES:
        qk = qk32.clone()
        qk[:, :DH] *= math.log2(math.e) / math.sqrt(hd)
        bufs[hd] = dict(qk=qk.to(bf), o=torch.zeros(M, DH, dtype=bf, device=dev), lse=torch.zeros(B, H, L, device=dev),
                        delta=torch.zeros(B, H, L, device=dev), dqk=torch.zeros(M, 2 * DH, dtype=bf, device=dev),
                        dqkv=torch.zeros(M, 3 * DH, dtype=bf, device=dev))
    del qk32
    unit = 2.0 * B * L * L * DH

    def fwd(hd, H):
        b = bufs[hd]
        return lambda: ops.flash_attn_fwd(b["qk"][:, :DH], b["qk"][:, DH:], qkv[:, 2 * DH:], b["o"], b["lse"], B, H, L, hd, 1 / math.sqrt(hd),
                                          q_prescaled=True)

    def bwd(hd, H):
        b = bufs[hd]
        return lambda: ops.flash_attn_bwd(b["qk"][:, :DH], b["qk"][:, DH:], qkv[:, 2 * DH:], b["o"], do, b["lse"], b["delta"], b["dqk"][:, :DH],
                                          b["dqk"][:, DH:], b["dqkv"][:, 2 * DH:], B, H, L, hd, 1 / math.sqrt(hd), q_prescaled=True)
    recs.append(compare("fwd_bf16_pre", {hd: fwd(hd, H) for hd, H in SIDES}, a.rounds, a.iters, 2 * unit))
    recs.append(compare("bwd_pair_bf16_pre", {hd: bwd(hd, H) for hd, H in SIDES}, a.rounds, a.iters, 7 * unit))
    del bufs, qkv, do

    # ---- the sampler's shape, forward: fp32, fp32-as-3-x-bf16, bf16
    B, L = 4, 1115
    unit = 2.0 * B * L * L * DH
    for tag, dtype, x3 in (("fp32", torch.float32, False), ("x3", torch.float32, True), ("bf16", bf, False)):
        M, qk32, qkv = problem(B, L, dtype, True)
        fns = {}
        for hd, H in SIDES:
            qk = qk32.clone()
            qk[:, :DH] *= math.log2(math.e) / math.sqrt(hd)
            qk = qk.to(dtype)
            o, lse = torch.zeros(M, DH, dtype=dtype, device=dev), torch.zeros(B, H, L, device=dev)
            fns[hd] = (lambda qk=qk, o=o, lse=lse, H=H, hd=hd, qkv=qkv: ops.flash_attn_fwd(
                qk[:, :DH], qk[:, DH:], qkv[:, 2 * DH:], o, lse, B, H, L, hd, 1 / math.sqrt(hd), x3=x3, q_prescaled=True))
        recs.append(compare(f"sampler_fwd_{tag}", fns, a.rounds, 4 * a.iters, 2 * unit))

    rec = {"tool": "tools/mb_attn_hd128.py", "device": torch.cuda.get_device_name(0), "kernel_src_sha": _lib.source_sha(),
           "lib": os.path.relpath(_lib.loaded_path()), "rounds": a.rounds, "iters": a.iters, "comparisons": recs}
    if a.out:
        os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(rec, f, indent=1)
    print(json.dumps({"kernel_src_sha": rec["kernel_src_sha"], **{r["name"]: round(r["ratio_128_over_64"], 4) for r in recs}}))


if __name__ == "__main__":
    main()
