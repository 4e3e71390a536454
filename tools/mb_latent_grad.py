"""What one forward + backward through the latent model costs on the HIP path, at the reference's training shape: the full model.yml
model (emb 6, style 32, 3 downs of stride 3, h_dim 128, 8 blocks per layer, expand 4, radius 2, 16 style heads of 64), 64 half-windows of
1026 frames, fp32 and bf16.  The work is the objective of tools/gen_latent_grad_golden.py (every path of the reference trainer's forward
without its losses): encode_chart, s swapped within pairs, model(audio, z + 0.2 noise, s), three pinned cotangents, backward to every
parameter.  Two forms alternate in one process, warmed up, timed with device events:

  (a) LatentModel on the HIP path (model.requires_grad_(True); bf16: compute_dtype = torch.bfloat16);
  (b) the same algorithm as torch-eager ops on the same GPU: autograd over the functional restatement below, which follows the
      reference's modules op for op (bf16: the forward under torch.autocast).

Both forms start from the same weights and inputs and print their objective, so a restatement that computed something else would show.

Prints JSON lines with the library's source hash.

  python tools/mb_latent_grad.py [--reps 5] [--steps 3] [--batch 64] [--frames 1026] [--layers 8]
"""
import argparse
import json
import os
import statistics
import sys

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--steps", type=int, default=3)
ap.add_argument("--batch", type=int, default=64)
ap.add_argument("--frames", type=int, default=1026)
ap.add_argument("--layers", type=int, default=8)
args = ap.parse_args()
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

from osu_dreamer_amd import _lib  # noqa: E402
from osu_dreamer_amd.latent import LatentModel  # noqa: E402
from tools.gen_latent_grad_golden import Case, grad_inputs, grad_weights, model_args, objective  # noqa: E402

dev = torch.device("cuda:0")
_lib.lib()
sha = _lib.source_sha()
HEAD_DIM, HEADS = 64, 16
c = Case(6, 32, 3, 3, 128, args.layers, 4, 2, HEAD_DIM, HEADS, args.batch, args.frames, args.batch, 1500, full=False)
W = grad_weights(c)
x = {k: v.to(dev) for k, v in grad_inputs(c).items()}


# ---------------------------------------------------------------- the model as torch-eager ops over a flat dict of parameters
def rms_norm(x, gamma=None):                      # common/rms_norm.py:6-16 (dim 1, eps 1e-6)
    y = x * x.pow(2).mean(dim=1, keepdim=True).add(1e-6).rsqrt()
    return y if gamma is None else y * gamma.view((-1,) + (1,) * (x.dim() - 2))


def spec_features(P, audio, p="audio_encoder.0.net."):                                   # spec_features.py:17-32
    x = F.conv2d(audio[:, None], P[p + "1.weight"], P[p + "1.bias"], stride=(6, 1), padding=(1, 1))
    x = F.silu(rms_norm(x, P[p + "2.gamma"]))
    x = F.conv2d(x, P[p + "4.weight"], P[p + "4.bias"], stride=(4, 1), padding=(1, 1))
    x = F.silu(rms_norm(x, P[p + "5.gamma"])).flatten(1, 2)
    return F.silu(rms_norm(F.conv1d(x, P[p + "8.weight"], P[p + "8.bias"]), P[p + "9.gamma"]))


def swiglu(P, p, x):                              # common/swiglu.py:27-32
    h = F.conv1d(x, P[p + "proj_vg.0.weight"], P[p + "proj_vg.0.bias"], padding=c.radius, groups=x.shape[1])
    v, g = F.conv1d(h, P[p + "proj_vg.1.weight"], P[p + "proj_vg.1.bias"]).chunk(2, dim=1)
    return F.conv1d(rms_norm(v * F.silu(g)), P[p + "proj_o.weight"], P[p + "proj_o.bias"])


def layer(P, p, x, cond):                         # unet.py:36-53
    for i in range(c.n_layers):
        scale = shift = gate = 0.0
        if cond is not None:
            scale, shift, gate = F.linear(cond, P[f"{p}films.{i}.weight"], P[f"{p}films.{i}.bias"])[:, :, None].chunk(3, dim=1)
        h = rms_norm(x, P[f"{p}norms.{i}.gamma"]) * (1 + scale) + shift
        x = x + rms_norm(swiglu(P, f"{p}blocks.{i}.0.", h), P[f"{p}blocks.{i}.1.gamma"]) * (1 + gate)
    return rms_norm(x, P[p + "out_norm.gamma"])


def unet_encoder(P, p, x):                        # unet.py:68-75
    skips = []
    for i in range(c.n_downs):
        x = layer(P, f"{p}layers.{i}.", x, None)
        skips.append(x)
        x = F.conv1d(x, P[f"{p}downs.{i}.0.weight"], P[f"{p}downs.{i}.0.bias"], padding=c.stride // 2, groups=x.shape[1])
        x = F.avg_pool1d(x, c.stride)
    return skips, x


def decode_logits(P, z, s, skips, p="decoder."):  # latent/model.py:103-114; unet.py:90-101, mixer :117-126
    x = F.conv1d(z, P["proj_emb.weight"], P["proj_emb.bias"])
    skips = list(skips)
    for i in range(c.n_downs):
        x = F.interpolate(x, scale_factor=c.stride, mode="nearest")
        x = F.conv1d(x, P[f"{p}ups.{i}.1.weight"], P[f"{p}ups.{i}.1.bias"], padding=c.stride // 2, groups=x.shape[1])
        skip, m = skips.pop().expand(x.shape[0], -1, -1), f"{p}mixers.{i}."
        proj = rms_norm(F.conv1d(skip, P[m + "proj.0.weight"], P[m + "proj.0.bias"]), P[m + "proj.1.gamma"])
        x = x + proj * F.conv1d(x, P[m + "gate.weight"], P[m + "gate.bias"])
        x = layer(P, f"{p}layers.{i}.", x, s)
    return F.conv1d(x, P["proj_out.weight"], P["proj_out.bias"])


def label_predictor(P, s):                        # latent/model.py:72-76
    return F.linear(F.silu(F.linear(s, P["label_predictor.0.weight"], P["label_predictor.0.bias"])),
                    P["label_predictor.2.weight"], P["label_predictor.2.bias"])


def attn_pool(P, p, x):                           # latent/model.py:23-36
    a = F.conv1d(x, P[p + "scores.weight"], P[p + "scores.bias"]).softmax(dim=-1)
    v = F.conv1d(x, P[p + "values.weight"], P[p + "values.bias"]).unflatten(1, (HEADS, -1))
    return F.linear(torch.einsum("bhl,bhdl->bhd", a, v).flatten(1), P[p + "proj_out.weight"], P[p + "proj_out.bias"])


def encode_chart(P, chart):                       # latent/model.py:93-101
    _, h = unet_encoder(P, "chart_encoder.1.", F.conv1d(chart, P["chart_encoder.0.weight"], P["chart_encoder.0.bias"]))
    s = rms_norm(attn_pool(P, "style_head.1.", layer(P, "style_head.0.", h, None)))
    return rms_norm(F.conv1d(layer(P, "temporal_layer.", h, s), P["temporal_head.0.weight"], P["temporal_head.0.bias"])), s


class Eager:
    """The restatement behind LatentModel's calls."""

    def __init__(self, autocast):
        self.P = {k: v.to(dev).requires_grad_(True) for k, v in W.items()}
        self.autocast = autocast

    def encode_chart(self, chart):
        return encode_chart(self.P, chart)

    def __call__(self, audio, z, s):
        skips, _ = unet_encoder(self.P, "audio_encoder.1.", spec_features(self.P, audio))
        return decode_logits(self.P, z, s, skips), label_predictor(self.P, s)

    def step(self):
        for p in self.P.values():
            p.grad = None
        with torch.autocast("cuda", dtype=torch.bfloat16, enabled=self.autocast):
            obj = objective(self, x)
        obj.backward()
        return obj


class Ours:
    def __init__(self, bf16):
        a = model_args(c)
        self.m = LatentModel(a["emb_dim"], a["style_dim"], a["n_downs"], a["stride"], a["args"])
        self.m.load_state_dict(W)
        self.m = self.m.to(dev)
        if bf16:
            self.m.compute_dtype = torch.bfloat16
        self.m.requires_grad_(True)

    def step(self):
        self.m.zero_grad(set_to_none=True)
        obj = objective(self.m, x)
        obj.backward()
        return obj


def timed(fn, n):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    for _ in range(n):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / n


for mode in ("fp32", "bf16"):
    forms = {"a_hip": Ours(mode == "bf16"), "b_torch_eager": Eager(mode == "bf16")}
    objs = {k: float(f.step().detach()) for k, f in forms.items()}           # warm-up: code objects, allocator, library algorithm choices
    for f in forms.values():
        f.step()
    torch.cuda.reset_peak_memory_stats()
    ms = {k: [] for k in forms}
    peak = {}
    for _ in range(args.reps):
        for k, f in forms.items():
            ms[k].append(timed(f.step, args.steps))
    for k, f in forms.items():
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        f.step()
        torch.cuda.synchronize()
        peak[k] = torch.cuda.max_memory_allocated() / 2 ** 30
    rec = {"tool": "mb_latent_grad", "kernel_src_sha": sha, "mode": mode, "B": c.B, "L": c.L, "n_layers": c.n_layers, "steps_per_rep": args.steps, "reps": args.reps}
    for k in forms:
        rec[k + "_ms"] = round(statistics.median(ms[k]), 2)
        rec[k + "_ms_min_max"] = [round(min(ms[k]), 2), round(max(ms[k]), 2)]
        rec[k + "_peak_gib"] = round(peak[k], 2)
        rec[k + "_objective"] = objs[k]
    rec["torch_over_hip"] = round(rec["b_torch_eager_ms"] / rec["a_hip_ms"], 3)
    print(json.dumps(rec), flush=True)
    del forms
    torch.cuda.empty_cache()
