"""Generate tests/golden/style_train_*.npz by running the REFERENCE's own StyleTrainer (osu_dreamer/models/style/train.py) on the CPU.

    python tools/gen_style_train_golden.py [out_dir]          (OSU_DREAMER_REFERENCE points at the reference checkout)

The fixtures hold inputs, the pinned random draws and recorded outputs only; weights are regenerated from a seed
(oracle.style_oracle.init_style_params — the reference's own zero-initialised films / proj_out.1 / u_out.weight would leave 20 of the 22
parameter tensors with an exactly zero gradient).  `style_batch`, `STYLE_MID` and the case table below are imported by the tests, which
never import the reference.

What the generator pins, and why:
  * torch.set_float32_matmul_precision("highest") AFTER constructing the trainer (its constructor sets "medium", which puts the
    reference's fp32 gradients 3.5e-3 from its own fp64 run; with "highest" they are within ~1e-6 per tensor);
  * the draws: the `th` name inside the reference's style/train.py is replaced by a stand-in whose randperm / rand / randn_like /
    rand_like return the recorded tensors; `th.randn` in style/model.py is patched for `sample`;
  * label masking: every label column of a single-step case has both masked and unmasked rows (asserted).
"""
from __future__ import annotations

import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
if REPO not in sys.path:
    sys.path.insert(0, REPO)

from oracle import style_oracle as SO  # noqa: E402

STYLE_MID = SO.StyleDims(style_dim=32, label_features=32, h_dim=128, depth=2, expand=4)
LABEL_DROP_PROB, OSL_W, DEL_W = 0.2, 1.0, 30.0
LR, WEIGHT_DECAY = 3e-4, 0.01
TRAJ_STEPS, TRAJ_WARMUP, TRAJ_DECAY_START = 40, 10, 25
SUB = 512                      # elements of the strided gradient sub-sample of the cases too wide to store whole gradients for

# name -> (dims, B, weight seed, batch seed)
STEP_CASES = {
    "style_train_step_tiny": (SO.STYLE_TINY, 6, 11, 0),
    "style_train_step_mid": (STYLE_MID, 48, 12, 0),
    "style_train_step_full": (SO.STYLE_FULL, 512, 13, 0),
}
TRAJ_CASES = {
    "style_train_traj40_tiny": (SO.STYLE_TINY, 6, 21, 100),
    "style_train_traj40_mid": (STYLE_MID, 48, 22, 200),
}
VAL_CASES = {
    "style_train_val_tiny": (SO.STYLE_TINY, 16, 31, 300),
}


def style_batch(d: SO.StyleDims, B: int, seed: int):
    """One training batch and the draws the step makes on it, from a seed: s1 (RMS-normalised codes, as encode-latents writes them),
    labels in [0, 10], and perm / r / s0 / drop in the order style/train.py:59-65 draws them.  `t` is what those make of perm and r."""
    g = torch.Generator().manual_seed(seed)
    s1 = torch.randn(B, d.style_dim, generator=g)
    s1 = s1 * torch.rsqrt(s1.square().mean(1, keepdim=True))
    labels = torch.rand(B, SO.NUM_LABELS, generator=g) * 10
    perm = torch.randperm(B, generator=g)
    r = torch.rand(B, generator=g)
    s0 = torch.randn(B, d.style_dim, generator=g)
    drop = torch.rand(B, SO.NUM_LABELS, generator=g)
    t = torch.special.ndtri(((perm + r) / B).clamp(1e-6, 1 - 1e-6)).sigmoid().to(torch.float32)
    return {"s1": s1, "labels": labels, "perm": perm, "r": r, "s0": s0, "drop": drop, "t": t}


def masks_every_column_both_ways(drop: torch.Tensor) -> bool:
    m = drop < LABEL_DROP_PROB
    return bool(m.any(0).all() and (~m).any(0).all())


def first_good_batch_seed(d, B, start):
    """The first seed >= start whose drop draws mask, and leave unmasked, some row of every label column."""
    for seed in range(start, start + 1000):
        if masks_every_column_both_ways(style_batch(d, B, seed)["drop"]):
            return seed
    raise AssertionError("no batch seed masks every label column both ways")


def sub(t: torch.Tensor, n: int = SUB) -> torch.Tensor:
    t = t.detach().flatten()
    return t[::max(1, t.numel() // n)][:n]


def np_dict(**kw):
    out = {}
    for k, v in kw.items():
        if isinstance(v, torch.Tensor):
            v = v.detach().cpu().numpy()
        out[k] = np.asarray(v)
    return out


# ---------------------------------------------------------------------------------------------------------------- reference side
class _PinnedTorch:
    """Stands in for the `th` name of the reference's style/train.py: the four draws return recorded tensors, the rest is torch."""

    def __init__(self, draws, dtype):
        self._d, self._dtype = draws, dtype

    def __getattr__(self, name):
        return getattr(torch, name)

    def randperm(self, n, **kw):
        assert n == self._d["perm"].numel()
        return self._d["perm"].clone()

    def rand(self, n, **kw):
        return self._d["r"].to(self._dtype)

    def randn_like(self, x):
        return self._d["s0"].to(x.dtype)

    def rand_like(self, x):
        return self._d["drop"].to(x.dtype)


def _reference():
    from oracle.make_golden import _install_shims
    _install_shims()
    import osu_dreamer.models.style.train as train_mod
    import osu_dreamer.models.style.model as model_mod
    from osu_dreamer.common.lr_schedule import LRScheduleArgs
    return train_mod, model_mod, LRScheduleArgs


def make_ref_trainer(d, seed, dtype=torch.float32, warmup=TRAJ_WARMUP, decay_start=TRAJ_DECAY_START):
    train_mod, model_mod, LRScheduleArgs = _reference()
    tr = train_mod.StyleTrainer(
        opt_args=dict(lr=LR, weight_decay=WEIGHT_DECAY),
        schedule_args=LRScheduleArgs(warmup_init=.3, warmup_steps=warmup, decay_start=decay_start),
        label_drop_prob=LABEL_DROP_PROB, osl_weight=OSL_W, del_weight=DEL_W, style_dim=d.style_dim,
        style_args=model_mod.StyleModelArgs(label_features=d.label_features, h_dim=d.h_dim, depth=d.depth, expand=d.expand))
    torch.set_float32_matmul_precision("highest")          # the constructor set "medium"
    P = SO.init_style_params(d, seed)
    assert sorted(tr.style.state_dict().keys()) == sorted(P.keys())
    tr.style.load_state_dict(P)
    tr.style_ema.module.load_state_dict(P)
    return tr.to(dtype), P


def ref_step(tr, batch, tag):
    """(loss, logs) of the reference's forward on `batch` with its draws pinned; tag: f32 | bf16 (forward under autocast) | f64."""
    train_mod, _, _ = _reference()
    dtype = torch.float64 if tag == "f64" else torch.float32
    saved = train_mod.th
    train_mod.th = _PinnedTorch(batch, dtype)
    try:
        B = batch["s1"].shape[0]
        args = (torch.empty(B, 0, 0), torch.empty(B, 0, 0), batch["s1"].to(dtype), batch["labels"].to(dtype))
        if tag == "bf16":
            with torch.autocast("cpu", dtype=torch.bfloat16):
                return tr(tr.style, *args)
        return tr(tr.style, *args)
    finally:
        train_mod.th = saved


def total_norm(grads):
    return float(torch.stack([g.double().norm() for g in grads.values()]).norm())


def gen_step(out_dir, name):
    d, B, wseed, bstart = STEP_CASES[name]
    bseed = first_good_batch_seed(d, B, bstart)
    batch = style_batch(d, B, bseed)
    assert masks_every_column_both_ways(batch["drop"])
    whole = d.h_dim <= 64
    fx = {"dims": np.array([d.style_dim, d.label_features, d.h_dim, d.depth, d.expand]), "seed": wseed, "batch_seed": bseed, "B": B,
          **{"in." + k: v for k, v in batch.items()}}
    grads = {}
    for tag in ("f32", "bf16", "f64"):
        tr, _ = make_ref_trainer(d, wseed, torch.float64 if tag == "f64" else torch.float32)
        loss, logs = ref_step(tr, batch, tag)
        loss.backward()
        g = {k: p.grad.detach().clone() for k, p in tr.style.named_parameters()}
        grads[tag] = g
        for k, v in logs.items():
            fx[f"{tag}.{k}"] = float(v)
        fx[f"{tag}.grad_norm"] = total_norm(g)
        for k, t in g.items():
            assert float(t.norm()) > 0, (name, tag, k)
            fx[f"{tag}.gradnorm.{k}"] = float(t.double().norm())
            fx[f"{tag}.{'grad' if whole else 'gradsub'}.{k}"] = (t if whole else sub(t)).float()
    worst = max(float((grads["f32"][k].double() - grads["f64"][k]).norm() / grads["f64"][k].norm()) for k in grads["f64"])
    assert worst < 1e-5, worst                     # the reference's own fp32 error on these inputs: far inside the tests' 1e-3
    fx["f32_vs_f64_worst"] = worst
    np.savez_compressed(os.path.join(out_dir, name + ".npz"), **np_dict(**fx))
    print(name, "batch seed", bseed, "loss", fx["f32.loss"], "f32 vs f64 worst grad", worst,
          "bf16 vs f32", min(float((grads["bf16"][k] - grads["f32"][k]).norm() / grads["f32"][k].norm()) for k in grads["f32"]),
          max(float((grads["bf16"][k] - grads["f32"][k]).norm() / grads["f32"][k].norm()) for k in grads["f32"]))


def gen_traj(out_dir, name):
    """40 optimizer steps: clip 1.0, AdamW, the schedule's warm-up / plateau / decay branches, EMA copy-then-lerp.  Recorded as
    traj40_*.npz is: loss, clip norm and LR per step; 64-element sub-samples of the final weights and EMA, their norms and moves."""
    d, B, wseed, bseed0 = TRAJ_CASES[name]
    fx = {"dims": np.array([d.style_dim, d.label_features, d.h_dim, d.depth, d.expand]), "seed": wseed, "batch_seed": bseed0, "B": B,
          "steps": TRAJ_STEPS, "warmup_steps": TRAJ_WARMUP, "decay_start": TRAJ_DECAY_START}
    sub64 = lambda w: sub(w.float(), 64)
    for tag in ("f32", "bf16"):
        tr, P0 = make_ref_trainer(d, wseed)
        cfg = tr.configure_optimizers()
        opt, sched = cfg["optimizer"], cfg["lr_scheduler"]["scheduler"]
        losses, norms, lrs = [], [], []
        for i in range(TRAJ_STEPS):
            batch = style_batch(d, B, bseed0 + i)
            lrs.append(opt.param_groups[0]["lr"])
            opt.zero_grad()
            loss, _ = ref_step(tr, batch, tag)
            loss.backward()
            norms.append(float(torch.nn.utils.clip_grad_norm_(tr.style.parameters(), 1.0)))
            opt.step()
            sched.step()
            tr.on_train_batch_end()
            losses.append(float(loss.detach()))
        fx[f"{tag}.loss"], fx[f"{tag}.grad_norm"], fx[f"{tag}.lr"] = np.array(losses), np.array(norms), np.array(lrs, dtype=np.float64)
        fx[f"{tag}.n_averaged"] = int(tr.style_ema.n_averaged)
        ema = dict(tr.style_ema.module.named_parameters())
        for k, p in tr.style.named_parameters():
            fx[f"{tag}.psub.{k}"], fx[f"{tag}.emasub.{k}"] = sub64(p), sub64(ema[k])
            fx[f"{tag}.pnorm.{k}"], fx[f"{tag}.emanorm.{k}"] = float(p.norm()), float(ema[k].norm())
            fx[f"{tag}.dnorm.{k}"] = float((p.detach() - P0[k]).norm())
        print(name, tag, "loss", losses[0], "->", losses[-1], "clip norm", norms[0], "->", norms[-1])
    np.savez_compressed(os.path.join(out_dir, name + ".npz"), **np_dict(**fx))


def gen_val(out_dir, name):
    """One validation epoch of the reference (train.py:111-150) on two batches: inputs, pins, the nine logged values in fp32, the K = 4
    sample sets, and the five sample metrics recomputed in fp64 from those samples."""
    train_mod, model_mod, _ = _reference()
    d, B, wseed, bseed = VAL_CASES[name]
    K = 4
    batch = style_batch(d, B, bseed)
    batch["labels"][:, 0] = torch.where(torch.arange(B) % 2 == 0, batch["labels"][:, 0] * 0.5 + 5.0, batch["labels"][:, 0] * 0.5)   # both sides of sr 5
    g = torch.Generator().manual_seed(bseed + 1)
    s_init = [torch.randn(B, d.style_dim, generator=g) for _ in range(K)]
    tr, _ = make_ref_trainer(d, wseed)
    logged = {}
    tr.log = lambda k, v, *a, **kw: logged.__setitem__(k, float(v))
    tr.log_dict = lambda dd, *a, **kw: logged.update({k: float(v) for k, v in dd.items()})
    samples = []
    queue = [s.clone() for s in s_init]
    real_sample = tr.style_ema.module.sample

    def sample(labels, n):
        out = real_sample(labels, n)
        samples.append(out.clone())
        return out
    tr.style_ema.module.sample = sample
    saved_th, saved_randn = train_mod.th, model_mod.th.randn
    train_mod.th = _PinnedTorch(batch, torch.float32)
    model_mod.th.randn = lambda *a, **kw: queue.pop(0)
    try:
        tr.on_validation_epoch_start()
        h = B // 2
        for i, sl in enumerate((slice(0, h), slice(h, B))):
            tr.validation_step((torch.empty(h, 0, 0), torch.empty(h, 0, 0), batch["s1"][sl], batch["labels"][sl]), i)
        with torch.no_grad():
            tr.on_validation_epoch_end()
    finally:
        train_mod.th, model_mod.th.randn = saved_th, saved_randn
    names = ["val/loss", "val/osl", "val/del", "val/u_mape", "val/nn_ratio", "val/nn_ratio_sr5", "val/cond_recall", "val/sample_spread", "val/energy_dist"]
    assert sorted(logged) == sorted(names), sorted(logged)
    samp = torch.stack(samples)
    # the same five metrics in fp64 from the same samples (this project's restatement of train.py:132-150, on double tensors)
    from osu_dreamer_amd.style_train import sample_metrics
    logged64 = {k: float(v) for k, v in sample_metrics(samp.double(), batch["s1"].double(), batch["labels"].double()).items()}
    for k in names[4:]:
        assert abs(logged[k] - logged64[k]) <= 1e-4 * abs(logged64[k]), (k, logged[k], logged64[k])
    fx = {"dims": np.array([d.style_dim, d.label_features, d.h_dim, d.depth, d.expand]), "seed": wseed, "batch_seed": bseed, "B": B, "K": K,
          **{"in." + k: v for k, v in batch.items()}, "s_init": torch.stack(s_init), "samples": samp,
          "sd_keys": np.array(sorted(tr.state_dict().keys()))}
    for k in names:
        fx["f32." + k] = logged[k]
    for k in names[4:]:
        fx["f64." + k] = logged64[k]
    np.savez_compressed(os.path.join(out_dir, name + ".npz"), **np_dict(**fx))
    print(name, logged)


def main():
    out_dir = sys.argv[1] if len(sys.argv) > 1 else os.path.join(REPO, "tests", "golden")
    torch.manual_seed(0)
    for name in STEP_CASES:
        gen_step(out_dir, name)
    for name in TRAJ_CASES:
        gen_traj(out_dir, name)
    for name in VAL_CASES:
        gen_val(out_dir, name)


if __name__ == "__main__":
    main()
