"""Generate tests/golden/latent_train_*.npz by running the REFERENCE's own LatentTrainer (osu_dreamer/models/latent/train.py) on the CPU.

    python tools/gen_latent_train_golden.py [out_dir]          (OSU_DREAMER_REFERENCE points at the reference checkout)

The fixtures hold inputs' seeds, the pinned draws' seeds and recorded results only.  Weights are `gen_latent_grad_golden.grad_weights` of
the cases `tiny`, `s4r1` and `wide` (their dims are the model's); batches and draws are rebuilt from seeds on both sides by `train_batch`
and `pins` (the tests import them, `TRAIN`, `trainer_kwargs` and the seed tables; they never import the reference).

What the generator pins, and why:
  * torch.set_float32_matmul_precision("highest") AFTER constructing the trainer (its constructor sets "medium");
  * the draws: the `th` name inside the reference's latent/train.py is replaced by a stand-in whose randn_like / rand hand out the recorded
    tensors in the order the forward asks for them (prior, eps_s, eps_z, repl; u_s, u_span, u_start);
  * the single-step pins are the first seed at which some rows of s are replaced and some are not, one row of z has span 0 and one a
    span >= 2 (asserted).  z_mask_frac is 0.75 here: at the reference's 0.25 the cases' 4..10 latent frames never give a span of 2.

Files:
  latent_train_step_<case>   the 13 logged values in fp64 / fp32 / bf16-autocast and every parameter gradient of the fp64 run (whole, or for
                             `wide` its norm and a 512-element sub-sample), with the reference's own fp32 and bf16 error per tensor
  latent_train_traj_tiny     10 steps of AdamW (clip 1.0, warm-up 4) in fp32 and fp64: loss per step, loss_ema after each step, the fp64 run's final
                             weights and per tensor the RMS distance of the fp32 run's from them
  latent_train_val_tiny      one validation epoch (eval mode) over two maps of different lengths: every logged value, fp32 and fp64; the
                             reference trainer's state-dict keys
"""
from __future__ import annotations

import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
for p in (REPO, HERE):
    if p not in sys.path:
        sys.path.insert(0, p)

from gen_latent_grad_golden import CASES, DEAD, ZERO_TRUE, Case, grad_weights, model_args, rel, sub, sub_err  # noqa: E402

TRAIN = dict(s_reg_weight=1e-3, s_noise=0.2, z_noise=0.2, s_mask_frac=0.3, z_mask_frac=0.75)
LR, WEIGHT_DECAY, WARMUP_INIT = 1e-3, 0.01, 0.1
BW = 3                                   # windows per batch: 6 half-window rows
STEP_CASES = {"tiny": 0, "s4r1": 0, "wide": 0}          # case -> first pin seed tried
TRAJ_STEPS, TRAJ_WARMUP, TRAJ_SEED = 10, 4, 5000
VAL_LENGTHS, VAL_SEED = (100, 131), 7000                # two maps, neither a multiple of 2 * chunk_size (18) nor of 54
LOG_NAMES = ("hit/onset", "hit/combo", "hit/slide", "hit/sustain", "hit/whistle", "hit/finish", "hit/clap", "cursor/pos", "cursor/vel",
             "cursor/acc", "label", "s_reg", "loss")
VAL_NAMES = tuple("val/" + n for n in LOG_NAMES) + ("eval/cursor_px_mae", "eval/label_mae", "eval/z_var_min", "eval/hit/dice",
                                                    "eval/cursor/vel/r2", "eval/score")


def half_len(c: Case) -> int:
    return 2 * c.L


def trainer_kwargs(c: Case, warmup: int = 0):
    """Constructor keywords of LatentTrainer on either side (schedule_args and latent_args as plain dicts)."""
    a = model_args(c)
    return dict(opt_args=dict(lr=LR, weight_decay=WEIGHT_DECAY), schedule_args=dict(warmup_init=WARMUP_INIT, warmup_steps=warmup), **TRAIN,
                emb_dim=a["emb_dim"], style_dim=a["style_dim"], n_downs=a["n_downs"], stride=a["stride"], latent_args=a["args"])


def train_batch(c: Case, seed: int, lengths=None):
    """(audio, chart, labels) of BW windows of two half-windows each (or one map per entry of `lengths`); the hit signals hold exact zeros
    and ones beside soft values, as real charts do."""
    g = torch.Generator().manual_seed(seed)

    def one(n, L):
        audio, chart = torch.randn(n, 72, L, generator=g), torch.rand(n, 9, L, generator=g)
        r = torch.rand(n, 7, L, generator=g)
        chart[:, :7][r < 0.4] = 0.0
        chart[:, :7][r > 0.9] = 1.0
        return audio, chart, torch.rand(n, 5, generator=g) * 10
    if lengths is None:
        return one(BW, 2 * half_len(c))
    return [one(1, L) for L in lengths]


def pins(c: Case, seed: int, B2: int = 2 * BW, l=None):
    """The draws of one forward, in the reference's order."""
    g = torch.Generator().manual_seed(seed)
    l = half_len(c) // c.stride ** c.n_downs if l is None else l
    return {"prior": torch.randn(B2, c.style, generator=g), "eps_s": torch.randn(B2, c.style, generator=g),
            "eps_z": torch.randn(B2, c.emb, l, generator=g), "u_s": torch.rand(B2, generator=g),
            "repl": torch.randn(B2, c.style, generator=g), "u_span": torch.rand(B2, generator=g), "u_start": torch.rand(B2, generator=g)}


def masks_of(c: Case, p):
    l = p["eps_z"].shape[-1]
    span = (p["u_span"] * TRAIN["z_mask_frac"] * l).long()
    return p["u_s"] < TRAIN["s_mask_frac"], span


def pins_are_good(c: Case, p) -> bool:
    masked, span = masks_of(c, p)
    return bool(masked.any() and (~masked).any() and (span == 0).any() and (span >= 2).any())


def first_good_pin_seed(c: Case, start: int) -> int:
    for seed in range(start, start + 1000):
        if pins_are_good(c, pins(c, seed)):
            return seed
    raise AssertionError("no pin seed masks some rows of s and gives spans 0 and >= 2")


# ---------------------------------------------------------------------------------------------------------------- reference side
class _PinnedTorch:
    """Stands in for the `th` name of the reference's latent/train.py: randn_like and rand hand out the recorded draws in call order."""

    def __init__(self, p, training):
        self._normal = [p["prior"]] + ([p["eps_s"], p["eps_z"], p["repl"]] if training else [])
        self._uniform = [p["u_s"], p["u_span"], p["u_start"]] if training else []

    def __getattr__(self, name):
        return getattr(torch, name)

    def randn_like(self, x):
        t = self._normal.pop(0)
        assert t.shape == x.shape, (t.shape, x.shape)
        return t.to(x.dtype)

    def rand(self, n, **kw):
        t = self._uniform.pop(0)
        assert t.numel() == n
        # the draws are fp32 numbers; the fp64 run takes the same numbers
        return t.clone()


def _reference():
    from oracle.make_golden import _install_shims
    if "osu_dreamer.models.latent.train" not in sys.modules:
        _install_shims()
        tb = types.ModuleType("torch.utils.tensorboard.writer")     # stand-in: plot_val, its only user, is not run
        tb.SummaryWriter = object
        sys.modules.setdefault("torch.utils.tensorboard", types.ModuleType("torch.utils.tensorboard"))
        sys.modules["torch.utils.tensorboard.writer"] = tb
    import osu_dreamer.models.latent.train as train_mod
    return train_mod


def make_ref_trainer(c: Case, dtype=torch.float32, warmup=0):
    train_mod = _reference()
    from osu_dreamer.common.lr_schedule import LRScheduleArgs
    from osu_dreamer.models.latent.model import LatentModelArgs
    from osu_dreamer.models.latent.unet import LayerArgs
    kw = trainer_kwargs(c, warmup)
    la = kw["latent_args"]
    kw["latent_args"] = LatentModelArgs(h_dim=la["h_dim"], ae_args=LayerArgs(**la["ae_args"]), style_head_dim=la["style_head_dim"],
                                        style_heads=la["style_heads"])
    kw["schedule_args"] = LRScheduleArgs(**kw["schedule_args"])
    tr = train_mod.LatentTrainer(**kw)
    torch.set_float32_matmul_precision("highest")          # the constructor set "medium"
    tr.latent.load_state_dict(grad_weights(c), strict=True)
    tr.plot_val = lambda b: None
    return tr.to(dtype)


def ref_forward(tr, batch, p, tag):
    """(loss, logs) of the reference's forward with its draws pinned; tag: f32 | bf16 (forward under autocast) | f64."""
    train_mod = _reference()
    dtype = torch.float64 if tag == "f64" else torch.float32
    saved = train_mod.th
    pinned = train_mod.th = _PinnedTorch(p, tr.training)
    try:
        b = train_mod.Batch(*(t.to(dtype) for t in batch))
        with torch.autocast("cpu", dtype=torch.bfloat16, enabled=tag == "bf16"):
            out = tr(b)
        assert not pinned._normal and not pinned._uniform, "draws left over"
        return out
    finally:
        train_mod.th = saved


def np_dict(fx):
    return {k: (v.detach().cpu().numpy() if isinstance(v, torch.Tensor) else np.asarray(v)) for k, v in fx.items()}


def gen_step(out_dir, name):
    c = CASES[name]
    pseed = first_good_pin_seed(c, STEP_CASES[name])
    p = pins(c, pseed)
    assert pins_are_good(c, p)
    batch = train_batch(c, c.seed + 10)
    fx = {"pin_seed": pseed, "batch_seed": c.seed + 10}
    grads = {}
    for tag in ("f64", "f32", "bf16"):
        tr = make_ref_trainer(c, torch.float64 if tag == "f64" else torch.float32).train()
        loss, logs = ref_forward(tr, batch, p, tag)
        loss.backward()
        grads[tag] = {k: q.grad for k, q in tr.latent.named_parameters()}
        assert tuple(logs) == LOG_NAMES
        fx[tag + ".logs"] = np.array([float(v) for v in logs.values()], dtype=np.float64)
        fx[tag + ".loss_ema"] = tr.loss_ema.double().numpy()
    dead = DEAD.format(c.n_downs - 1)
    worst32 = 0.0
    for k, g in grads["f64"].items():
        if k.startswith(dead):
            assert g is None, k
            continue
        assert float(g.norm()) > 0 or k == ZERO_TRUE, k
        fx["n64." + k] = np.float64(float(g.norm()))
        if c.full:
            fx["g64." + k] = g.to(torch.float32).numpy()
        else:
            fx["s64." + k] = sub(g).to(torch.float32).numpy()
        for tag, key in (("f32", "32"), ("bf16", "bf")):
            gg = grads[tag][k]
            fx[f"n{key}." + k] = np.float64(float(gg.norm()))
            err = float(gg.norm()) if k == ZERO_TRUE else rel(gg, g) if c.full else sub_err(gg, sub(g), g.norm())
            fx[f"err{key}." + k] = np.float64(err)
        if k != ZERO_TRUE:
            worst32 = max(worst32, float(fx["err32." + k]))
    assert worst32 < 1e-4, worst32          # the reference's own fp32 error: far inside the tests' 1e-3
    np.savez_compressed(os.path.join(out_dir, f"latent_train_step_{name}.npz"), **np_dict(fx))
    masked, span = masks_of(c, p)
    print(f"step {name}: pin seed {pseed}, masked {masked.tolist()}, spans {span.tolist()}, loss {fx['f64.logs'][-1]:.6f}, "
          f"reference fp32 vs fp64 worst gradient {worst32:.2e}")


def traj_inputs(c: Case, i: int):
    return train_batch(c, TRAJ_SEED + 10 * i), pins(c, TRAJ_SEED + 10 * i + 1)


def gen_traj(out_dir, name="tiny"):
    c = CASES[name]
    fx, final = {"steps": TRAJ_STEPS, "warmup_steps": TRAJ_WARMUP}, {}
    for tag in ("f32", "f64"):
        tr = make_ref_trainer(c, torch.float64 if tag == "f64" else torch.float32, warmup=TRAJ_WARMUP).train()
        (opt,), (sched,) = tr.configure_optimizers()
        sched = sched["scheduler"]
        losses, emas, lrs = [], [], []
        for i in range(TRAJ_STEPS):
            batch, p = traj_inputs(c, i)
            lrs.append(opt.param_groups[0]["lr"])
            opt.zero_grad()
            loss, _ = ref_forward(tr, batch, p, tag)
            loss.backward()
            torch.nn.utils.clip_grad_norm_(tr.parameters(), 1.0)
            opt.step()
            sched.step()
            losses.append(float(loss.detach()))
            emas.append(tr.loss_ema.double().numpy().copy())
        fx[tag + ".loss"], fx[tag + ".loss_ema"], fx[tag + ".lr"] = np.array(losses), np.stack(emas), np.array(lrs, dtype=np.float64)
        final[tag] = {k: q.detach().double() for k, q in tr.latent.named_parameters()}
        print(f"traj {name} {tag}: loss {losses[0]:.6f} -> {losses[-1]:.6f}")
    for k, w in final["f64"].items():          # the fp64 run's weights (as fp32) and the RMS distance of the fp32 run's from them
        fx["f64.w." + k] = w.to(torch.float32).numpy()
        fx["dist." + k] = np.float64(float((final["f32"][k] - w).pow(2).mean().sqrt()))
    np.savez_compressed(os.path.join(out_dir, f"latent_train_traj_{name}.npz"), **np_dict(fx))


def val_inputs(c: Case):
    maps = train_batch(c, VAL_SEED, lengths=VAL_LENGTHS)
    cs = 2 * c.stride ** c.n_downs
    ps = [pins(c, VAL_SEED + 1 + i, B2=2, l=-(-L // cs) * cs // (2 * c.stride ** c.n_downs)) for i, L in enumerate(VAL_LENGTHS)]
    return maps, ps


def gen_val(out_dir, name="tiny"):
    train_mod = _reference()
    c = CASES[name]
    assert all(L % 54 and L % (2 * c.stride ** c.n_downs) for L in VAL_LENGTHS) and len(set(VAL_LENGTHS)) == len(VAL_LENGTHS)
    maps, ps = val_inputs(c)
    fx = {}
    for tag in ("f32", "f64"):
        dtype = torch.float64 if tag == "f64" else torch.float32
        tr = make_ref_trainer(c, dtype).eval()
        steps, end = [], {}
        tr.log_dict = lambda d, *a, **kw: steps[-1].update({k: float(v) for k, v in d.items()})
        tr.on_validation_epoch_start()
        saved = train_mod.th
        try:
            for i, (m, p) in enumerate(zip(maps, ps)):
                steps.append({})
                b = tr.on_after_batch_transfer(train_mod.Batch(*(t.to(dtype) for t in m)), 0)
                train_mod.th = _PinnedTorch(p, False)
                tr.validation_step(b, i)
        finally:
            train_mod.th = saved
        tr.log_dict = lambda d, *a, **kw: end.update({k: float(v) for k, v in d.items()})
        tr.on_validation_epoch_end()
        vals = {k: float(np.mean([s[k] for s in steps])) for k in steps[0]}
        vals.update(end)
        assert sorted(vals) == sorted(VAL_NAMES), sorted(vals)
        fx[tag] = np.array([vals[k] for k in VAL_NAMES], dtype=np.float64)
        fx["sd_keys"] = np.array(sorted(tr.state_dict().keys()))
        print(f"val {name} {tag}:", {k: round(vals[k], 6) for k in VAL_NAMES[-6:]})
    np.savez_compressed(os.path.join(out_dir, f"latent_train_val_{name}.npz"), **np_dict(fx))


def main():
    out_dir = sys.argv[1] if len(sys.argv) > 1 else os.path.join(REPO, "tests", "golden")
    for name in STEP_CASES:
        gen_step(out_dir, name)
    gen_traj(out_dir)
    gen_val(out_dir)
    for f in sorted(os.listdir(out_dir)):
        if f.startswith("latent_train_"):
            assert os.path.getsize(os.path.join(out_dir, f)) < (1 << 20), f


if __name__ == "__main__":
    main()
