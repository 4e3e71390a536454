"""What the style model's training step costs on the HIP path: full model (style_dim 32, label_features 128, h_dim 256, depth 8, expand 4),
B = 512, fp32 and bf16, one whole step each (zero_grad, forward + loss, backward, clip + AdamW + EMA), warmed up, device-synchronised,
the three forms alternating in one process:

  (a) StyleTrainer, eager launches;
  (b) StyleTrainer with the step captured into one hipGraph (use_graph);
  (c) the same algorithm as torch-eager ops on the same GPU: autograd over oracle.style_oracle.style_forward, the loss of
      style/train.py:69-81, clip_grad_norm_, torch.optim.AdamW and an EMA lerp (bf16: the forward under torch.autocast).

Then, per product class of the step, the forward launch through od_linear_small (fp32) and through od_gemm_nt (fp32 and bf16), and the
backward through od_linear_small_bwd and through od_gemm_tn + od_gemm_nt, with which of them the step uses.
Prints JSON lines with the library's source hash.

  python tools/mb_style_train.py [--reps 7] [--steps 20] [--batch 512]
"""
import argparse
import json
import os
import statistics
import sys
import time

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=7)
ap.add_argument("--steps", type=int, default=20)
ap.add_argument("--batch", type=int, default=512)
args = ap.parse_args()
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

from oracle import style_oracle as SO  # noqa: E402
from osu_dreamer_amd import _lib, ops  # noqa: E402
from osu_dreamer_amd._lib import OD_ACT_NONE  # noqa: E402
from osu_dreamer_amd.lr_schedule import LRScheduleArgs  # noqa: E402
from osu_dreamer_amd.style import StyleModel  # noqa: E402
from osu_dreamer_amd.style_train import StyleTrainer  # noqa: E402
from tools.gen_style_train_golden import style_batch  # noqa: E402

dev = torch.device("cuda:0")
_lib.lib()
sha = _lib.source_sha()
d, B = SO.STYLE_FULL, args.batch
P = SO.init_style_params(d, 1)
batch = {k: v.to(dev) for k, v in style_batch(d, B, 2).items()}
c0, u_scale = SO.style_constants(d.style_dim)


def timed(fn, n):
    torch.cuda.synchronize()
    t = time.perf_counter()
    for _ in range(n):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t) / n


def ours(use_graph, dtype):
    tr = StyleTrainer(opt_args=dict(lr=3e-4, weight_decay=0.01), schedule_args=LRScheduleArgs(), label_drop_prob=.2, osl_weight=1.,
                      del_weight=30., style_dim=d.style_dim,
                      style_args=dict(label_features=d.label_features, h_dim=d.h_dim, depth=d.depth, expand=d.expand))
    tr.style.load_state_dict(P)
    tr.style_ema.module.load_state_dict(P)
    tr = tr.to(dev)
    tr.use_graph, tr.gradient_clip_val, tr.style.compute_dtype = use_graph, 1.0, dtype
    opt = tr.configure_optimizers()["optimizer"]

    def step():
        opt.zero_grad()
        loss, _ = tr(tr.style, None, None, batch["s1"], batch["labels"], t=batch["t"], s0=batch["s0"], drop=batch["drop"])
        loss.backward()
        opt.step()
        tr.on_train_batch_end()
    return step


def torch_eager(dtype):
    W = {k: v.clone().to(dev).requires_grad_(not k.startswith("rff.")) for k, v in P.items()}
    params = [v for k, v in W.items() if v.requires_grad]
    ema = [p.detach().clone() for p in params]
    opt = torch.optim.AdamW(params, lr=3e-4, weight_decay=0.01)

    def step():
        opt.zero_grad()
        s1 = batch["s1"]
        st = torch.lerp(batch["s0"], s1, batch["t"][:, None])
        labels = torch.where(batch["drop"] < .2, -1.0, batch["labels"])
        with torch.autocast("cuda", dtype=torch.bfloat16, enabled=dtype == torch.bfloat16):
            u, v = SO.style_forward(st, labels, W, d)
        u, v = u.float(), v.float()
        d_sq = (st - s1).square().sum(1)
        u_t = (d_sq + c0).sqrt()
        osl = ((st - u[:, None] * v - s1).square().sum(1) / (d_sq + c0)).mean()
        del_ = (v - (st - s1) / u_t[:, None]).square().sum(1).mean()
        (osl + 30. * del_).backward()
        torch.nn.utils.clip_grad_norm_(params, 1.0)
        opt.step()
        with torch.no_grad():
            torch._foreach_lerp_(ema, [p.detach() for p in params], 0.01)
    return step


for name, dtype in (("fp32", torch.float32), ("bf16", torch.bfloat16)):
    forms = {"a_eager": ours(False, dtype), "b_graph": ours(True, dtype), "c_torch_eager": torch_eager(dtype)}
    for f in forms.values():
        for _ in range(3):
            f()
    times = {k: [] for k in forms}
    for _ in range(args.reps):
        for k, f in forms.items():
            times[k].append(timed(f, args.steps))
    rec = {"tool": "mb_style_train", "kernel_src_sha": sha, "mode": name, "B": B, "steps_per_rep": args.steps}
    for k, ts in times.items():
        rec[k + "_us"] = round(statistics.median(ts) * 1e6, 1)
        rec[k + "_us_min_max"] = [round(min(ts) * 1e6, 1), round(max(ts) * 1e6, 1)]
    rec["graph_over_eager"] = round(rec["a_eager_us"] / rec["b_graph_us"], 3)
    rec["torch_over_best"] = round(rec["c_torch_eager_us"] / min(rec["a_eager_us"], rec["b_graph_us"]), 3)
    print(json.dumps(rec), flush=True)

# ---- per product class: which entry point, and what it costs
H, X, S = d.h_dim, d.expand * d.h_dim, d.style_dim
GEMM32 = f"od_gemm_nt / od_gemm_tn in fp32 (B >= {StyleModel.gemm_min_rows} rows; od_linear_small below)"
CLASSES = (("blocks.i.0", X, H, "fp32: " + GEMM32 + "; bf16: od_gemm_nt / od_gemm_tn in bf16"),
           ("blocks.i.3", H, X, "fp32: " + GEMM32 + "; bf16: od_gemm_nt / od_gemm_tn in bf16"),
           ("films.i", 3 * H, H, GEMM32 + " in both modes (fp32 output read by the norm kernels)"),
           ("proj_in", H, S, GEMM32 + " in both modes"), ("proj_out.1", S, H, GEMM32 + " in both modes"))
g = torch.Generator().manual_seed(0)
for cname, N, K, used in CLASSES:
    x, w, b = torch.randn(B, K, generator=g).to(dev), (torch.randn(N, K, generator=g) / K ** .5).to(dev), torch.zeros(N, device=dev)
    dout = torch.randn(B, N, generator=g).to(dev)
    out, dpre, dW, db, dx = (torch.empty(B, N, device=dev), torch.empty(B, N, device=dev), torch.zeros(N, K, device=dev),
                             torch.zeros(N, device=dev), torch.empty(B, K, device=dev))
    rec = {"tool": "mb_style_train", "kernel_src_sha": sha, "product": cname, "M": B, "N": N, "K": K, "step_uses": used}
    rec["fwd_linear_small_us"] = round(timed(lambda: ops.linear_small(x, w, b, out), 50) * 1e6, 1)
    rec["bwd_linear_small_us"] = round(timed(lambda: ops.linear_small_bwd(x, w, None, dout, dpre, dW, db, dx, False, OD_ACT_NONE), 50) * 1e6, 1)
    for tag, dt in (("f32", torch.float32), ("bf16", torch.bfloat16)):
        if K % 8 or N % 8:
            continue
        xa, wa, wT, oa, da, dxa = x.to(dt), w.to(dt), w.t().contiguous().to(dt), torch.empty(B, N, device=dev, dtype=dt), dout.to(dt), \
            torch.empty(B, K, device=dev, dtype=dt)
        rec[f"fwd_gemm_nt_{tag}_us"] = round(timed(lambda: ops.gemm_nt(xa, wa, b, oa), 50) * 1e6, 1)

        def bwd():
            ops.gemm_tn(da, xa, dW, dbias=db)
            ops.gemm_nt(da, wT, None, dxa)
        rec[f"bwd_gemm_tn_nt_{tag}_us"] = round(timed(bwd, 50) * 1e6, 1)
    print(json.dumps(rec), flush=True)
