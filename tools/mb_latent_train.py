"""What one training step of the latent model (forward, loss, backward) costs, at the reference's training shape: the full latent.yml model,
64 half-windows of 1026 frames (32 windows of 2052), fp32 and bf16, in three forms that alternate in one process, warmed up, timed with
device events, medians of --reps repetitions:

  (a) LatentTrainer of this package: LatentModel on the HIP path under od_mmd_imq / od_latent_perturb / od_latent_loss;
  (b) the same LatentModel under the reference trainer's forward written as torch-eager ops (the recipe of INTEGRATION.md: cdist-based
      MMD, the eager perturbation and losses, the host read of loss_ema_initialized);
  (c) everything as torch-eager ops: the functional restatement of the model from tools/mb_latent_grad.py under the same eager loss
      (bf16: the model's forward under torch.autocast).

All three start from the same weights, batch and pinned draws and print their loss, so a form that computed something else would show.
Prints JSON lines with the library's source hash.

  python tools/mb_latent_train.py [--reps 5] [--steps 3] [--windows 32] [--frames 1026] [--layers 8]
"""
import argparse
import json
import os
import statistics
import sys

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--steps", type=int, default=3)
ap.add_argument("--windows", type=int, default=32)
ap.add_argument("--frames", type=int, default=1026)
ap.add_argument("--layers", type=int, default=8)
args = ap.parse_args()
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

from osu_dreamer_amd import _lib  # noqa: E402
from osu_dreamer_amd.latent_train import LOG_NAMES, LOSS_COMPONENT_WEIGHTS, LatentTrainer, split_halves  # noqa: E402
from tools.gen_latent_grad_golden import Case, grad_weights, model_args  # noqa: E402

dev = torch.device("cuda:0")
_lib.lib()
sha = _lib.source_sha()
HEAD_DIM, HEADS = 64, 16
B2 = 2 * args.windows
c = Case(6, 32, 3, 3, 128, args.layers, 4, 2, HEAD_DIM, HEADS, B2, args.frames, B2, 1500, full=False)
W = grad_weights(c)
TRAIN = dict(s_reg_weight=1e-3, s_noise=0.2, z_noise=0.2, s_mask_frac=0.1, z_mask_frac=0.25)          # latent.yml
g = torch.Generator().manual_seed(c.seed + 2)
l = c.L // c.stride ** c.n_downs
chart = torch.rand(args.windows, 9, 2 * c.L, generator=g)
chart[:, :7][torch.rand(args.windows, 7, 2 * c.L, generator=g) < 0.5] = 0.0
batch = tuple(t.to(dev) for t in (torch.randn(args.windows, 72, 2 * c.L, generator=g), chart, 10 * torch.rand(args.windows, 5, generator=g)))
pins = {k: v.to(dev) for k, v in dict(
    prior=torch.randn(B2, c.style, generator=g), eps_s=torch.randn(B2, c.style, generator=g), eps_z=torch.randn(B2, c.emb, l, generator=g),
    u_s=torch.rand(B2, generator=g), repl=torch.randn(B2, c.style, generator=g), u_span=torch.rand(B2, generator=g),
    u_start=torch.rand(B2, generator=g)).items()}


# ---------------------------------------------------------------- the model as torch-eager ops over a flat dict of parameters
# (the restatement of tools/mb_latent_grad.py, which runs on import and so cannot be imported)
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


# ---------------------------------------------------------------- the reference trainer's forward as torch-eager ops
def mmd_imq(z, z_prior):                          # common/wae.py:4-28
    n, d = z.shape

    def kernel(a, b):
        d2 = torch.cdist(a, b).pow(2)
        out = torch.zeros_like(d2)
        for s in (.1, .2, .5, 1., 2., 5., 10.):
            out = out + 2. * d * s / (2. * d * s + d2)
        return out
    off = 1. - torch.eye(n, device=z.device, dtype=z.dtype)
    return (kernel(z, z) * off).sum() / (n * (n - 1)) + (kernel(z_prior, z_prior) * off).sum() / (n * (n - 1)) - 2. * kernel(z, z_prior).mean()


class EagerLoss:
    """latent/train.py:75-154 over any model with encode_chart and __call__, draws pinned; keeps loss_ema and its flag as the reference does."""

    def __init__(self):
        self.loss_ema = torch.ones(len(LOSS_COMPONENT_WEIGHTS), device=dev)
        self.loss_ema_initialized = torch.tensor(False, device=dev)

    def __call__(self, model):
        audio, true_chart, true_labels = split_halves(batch[0]), split_halves(batch[1]), batch[2].repeat_interleave(2, dim=0)
        z, s = model.encode_chart(true_chart)
        s_reg = mmd_imq(s, pins["prior"])
        s = s.view(-1, 2, s.shape[1]).flip(1).reshape(s.shape)
        s = s + TRAIN["s_noise"] * pins["eps_s"]
        z = z + TRAIN["z_noise"] * pins["eps_z"]
        s_masked = pins["u_s"] < TRAIN["s_mask_frac"]
        s = torch.where(s_masked[:, None], pins["repl"], s)
        span = (pins["u_span"] * TRAIN["z_mask_frac"] * z.shape[2]).long()
        start = (pins["u_start"] * (z.shape[2] - span).clamp(min=1)).long()
        idx = torch.arange(z.shape[2], device=dev)[None]
        z = z.masked_fill(((idx >= start[:, None]) & (idx < (start + span)[:, None]))[:, None, :], 0.)
        logits, pred_labels = model(audio, z, s)
        logits, pred_labels = logits.float(), pred_labels.float()
        th = true_chart[:, :7]
        floor = -torch.special.xlogy(th, th) - torch.special.xlogy(1 - th, 1 - th)
        hit = (F.binary_cross_entropy_with_logits(logits[:, :7], th, reduction="none") - floor).mean(dim=(0, 2))
        cursor = [F.mse_loss(logits[:, 7:].diff(n=i), true_chart[:, 7:].diff(n=i)) for i in range(3)]
        label = torch.where(s_masked, 0., (pred_labels - true_labels).pow(2).mean(dim=1)).sum() / (~s_masked).sum().clamp(min=1)
        losses = torch.stack([*hit.unbind(), *cursor, label])
        if not self.loss_ema_initialized:
            self.loss_ema.copy_(losses.detach())
            self.loss_ema_initialized.fill_(True)
        else:
            self.loss_ema.lerp_(losses.detach(), 0.01)
        weights = losses.new_tensor(list(LOSS_COMPONENT_WEIGHTS.values()))
        return (weights * losses / self.loss_ema.clamp(min=1e-8)).sum() + TRAIN["s_reg_weight"] * s_reg


class Eager:
    """The restatement behind LatentModel's calls."""

    def __init__(self, autocast):
        self.P = {k: v.to(dev).requires_grad_(True) for k, v in W.items()}
        self.autocast = autocast

    def encode_chart(self, chart):
        with torch.autocast("cuda", dtype=torch.bfloat16, enabled=self.autocast):
            z, s = encode_chart(self.P, chart)
        return z.float(), s.float()

    def __call__(self, audio, z, s):
        with torch.autocast("cuda", dtype=torch.bfloat16, enabled=self.autocast):
            skips, _ = unet_encoder(self.P, "audio_encoder.1.", spec_features(self.P, audio))
            return decode_logits(self.P, z, s, skips), label_predictor(self.P, s)


def trainer(bf16):
    a = model_args(c)
    tr = LatentTrainer(opt_args=dict(lr=1e-3, weight_decay=0.01), schedule_args=dict(warmup_init=0.1, warmup_steps=2000), **TRAIN,
                       emb_dim=a["emb_dim"], style_dim=a["style_dim"], n_downs=a["n_downs"], stride=a["stride"], latent_args=a["args"])
    tr.latent.load_state_dict(W)
    tr = tr.to(dev).train()
    if bf16:
        tr.latent.compute_dtype = torch.bfloat16
    return tr


class FormA:
    def __init__(self, bf16):
        self.tr = trainer(bf16)

    def step(self):
        self.tr.latent.zero_grad(set_to_none=True)
        loss, _ = self.tr(batch, **pins)
        loss.backward()
        return loss


class FormB:
    def __init__(self, bf16):
        self.m, self.loss = trainer(bf16).latent, EagerLoss()

    def step(self):
        self.m.zero_grad(set_to_none=True)
        loss = self.loss(self.m)
        loss.backward()
        return loss


class FormC:
    def __init__(self, bf16):
        self.m, self.loss = Eager(bf16), EagerLoss()

    def step(self):
        for p in self.m.P.values():
            p.grad = None
        loss = self.loss(self.m)
        loss.backward()
        return loss


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
    forms = {"a_trainer": FormA(mode == "bf16"), "b_hip_model_eager_loss": FormB(mode == "bf16"), "c_all_torch_eager": FormC(mode == "bf16")}
    first = {k: float(f.step().detach()) for k, f in forms.items()}           # warm-up: code objects, allocator, library algorithm choices
    for f in forms.values():
        f.step()
    ms = {k: [] for k in forms}
    for _ in range(args.reps):
        for k, f in forms.items():
            ms[k].append(timed(f.step, args.steps))
    rec = {"tool": "mb_latent_train", "kernel_src_sha": sha, "mode": mode, "rows": B2, "L": c.L, "n_layers": c.n_layers,
           "steps_per_rep": args.steps, "reps": args.reps}
    for k in forms:
        rec[k + "_ms"] = round(statistics.median(ms[k]), 2)
        rec[k + "_ms_min_max"] = [round(min(ms[k]), 2), round(max(ms[k]), 2)]
        rec[k + "_first_loss"] = first[k]
    rec["b_minus_a_ms"] = round(rec["b_hip_model_eager_loss_ms"] - rec["a_trainer_ms"], 2)
    rec["c_over_a"] = round(rec["c_all_torch_eager_ms"] / rec["a_trainer_ms"], 3)
    print(json.dumps(rec), flush=True)
    del forms
    torch.cuda.empty_cache()
