"""`LatentTrainer` on the HIP path against the reference's own LatentTrainer (tests/golden/latent_train_*.npz, recorded by
tools/gen_latent_train_golden.py from osu_dreamer/models/latent/train.py in fp64, fp32 and under bf16 autocast, every random draw pinned).

Rules:
  single pinned step     the 13 logged values within 2e-5 relative of the reference's fp64 values (fp32); every parameter gradient within 1e-3
                         relative L2 of the fp64 one in fp32, and in bf16 within 3 x the reference's own bf16-autocast error on that tensor
                         (test_latent_grad.py's rules, its treatment of style_head.1.scores.bias and of the last audio down-conv included).
                         `wide` runs on the GPU only and is known by norms and sub-samples.
  ten AdamW steps        loss within 1e-4 relative at every step; final weights, per tensor, RMS distance from the reference's fp64 run
                         <= the larger of test_trajectory.py's rule (1e-5 rms|w| + 1e-3 rms|w - w0| + 1e-7) and 3 x the distance between
                         the reference's own fp32 and fp64 runs
  validation epoch       every returned value within 1e-4 relative of the fp64 run
  state dict             the reference's keys; loss_ema_initialized stays torch.bool; save -> load continues a trajectory bit for bit
                         (deterministic mode: the shared GEMM backwards add with atomics otherwise)
  eval forward           bit-identical across calls with the same prior
  no host sync           steps 2 and 3 run under torch.cuda.set_sync_debug_mode("error") (GPU only)
"""
import os

import numpy as np
import pytest
import torch

from osu_dreamer_amd import det
from osu_dreamer_amd.latent_train import LOG_NAMES, LatentTrainer
from tools.gen_latent_train_golden import (CASES, DEAD, TRAJ_STEPS, TRAJ_WARMUP, VAL_NAMES, ZERO_TRUE, grad_weights, pins, sub_err, train_batch,
                                           traj_inputs, trainer_kwargs, val_inputs)
from tools.gen_latent_train_golden import LOG_NAMES as REF_LOG_NAMES
from kernel_backend import dev, rel_l2  # noqa: F401

GOLDEN = os.path.join(os.path.dirname(__file__), "golden")
SCORES_W = "style_head.1.scores.weight"


def load(name):
    z = np.load(os.path.join(GOLDEN, name + ".npz"))
    return {k: (z[k] if z[k].dtype.kind == "U" else torch.from_numpy(np.asarray(z[k]))) for k in z.files}


def make(name, device, bf16=False, warmup=0):
    c = CASES[name]
    if device.type == "cpu" and c.h_dim > 64:
        pytest.skip("the full-width latent model runs on the GPU only")
    tr = LatentTrainer(**trainer_kwargs(c, warmup))
    tr.latent.load_state_dict(grad_weights(c))
    tr = tr.to(device)
    if bf16:
        tr.latent.compute_dtype = torch.bfloat16
    return c, tr


def on(batch, device):
    return tuple(t.to(device) for t in batch)


def test_log_names_are_the_references():
    assert tuple(LOG_NAMES) == tuple(REF_LOG_NAMES) and len(LOG_NAMES) == 13


@pytest.mark.parametrize("mode", ["fp32", "bf16"])
@pytest.mark.parametrize("name", ["tiny", "s4r1", "wide"])
def test_single_pinned_step(dev, name, mode):
    c, tr = make(name, dev, bf16=mode == "bf16")
    fx = load("latent_train_step_" + name)
    batch, p = train_batch(c, int(fx["batch_seed"])), pins(c, int(fx["pin_seed"]))
    tr.train()
    loss, logs = tr(on(batch, dev), **p)
    loss.backward()
    assert tuple(logs) == tuple(LOG_NAMES) and torch.equal(loss.detach(), logs["loss"])
    got = torch.stack([logs[k] for k in LOG_NAMES]).double().cpu()
    err = ((got - fx["f64.logs"]).abs() / fx["f64.logs"].abs())
    print(f"{name} {mode}: logs' relative errors {[f'{float(e):.1e}' for e in err]}")
    if mode == "fp32":
        assert bool((err <= 2e-5).all()), dict(zip(LOG_NAMES, err.tolist()))
        assert rel_l2(tr.loss_ema, fx["f64.loss_ema"]) <= 2e-5 and bool(tr.loss_ema_initialized)
    else:
        assert bool(torch.isfinite(got).all())
    dead = DEAD.format(c.n_downs - 1)
    grads = {k: q.grad for k, q in tr.latent.named_parameters()}
    worst = ("", 0.0)
    for k, g in grads.items():
        if k.startswith(dead):
            assert g is None or not bool(g.any()), f"{k}: the conv that feeds only h got a gradient"
            continue
        assert g is not None and g.dtype == torch.float32 and bool(torch.isfinite(g).all()), k
        if k == ZERO_TRUE:
            lim = 1e-5 * float(grads[SCORES_W].norm()) if mode == "fp32" else 3 * float(fx["errbf." + k])
            assert float(g.norm()) <= lim, (k, float(g.norm()), lim)
            continue
        err = rel_l2(g, fx["g64." + k]) if c.full else sub_err(g.cpu(), fx["s64." + k], fx["n64." + k])
        lim = 1e-3 if mode == "fp32" else 3 * float(fx["errbf." + k])
        print(f"{name} {mode} {k}: {err:.3e} (limit {lim:.3e})")
        assert err <= lim, (k, err, lim)
        worst = max(worst, (k, err / lim), key=lambda t: t[1])
    print(f"[{name}/{mode}] worst {worst[0]} at {worst[1]:.3f} of its limit")


def run_steps(tr, c, device, first, last, opt=None, sched=None):
    if opt is None:
        tr.gradient_clip_val = 1.0
        cfg = tr.configure_optimizers()
        opt, sched = cfg["optimizer"], cfg["lr_scheduler"]["scheduler"]
    tr.train()
    losses, emas, lrs = [], [], []
    for i in range(first, last):
        batch, p = traj_inputs(c, i)
        lrs.append(opt.param_groups[0]["lr"])
        opt.zero_grad()
        loss = tr.training_step(on(batch, device), i, **p)
        loss.backward()
        opt.step()
        sched.step()
        losses.append(loss.detach().clone())
        emas.append(tr.loss_ema.detach().clone())
    return losses, emas, lrs, opt, sched


def test_ten_step_trajectory(dev):
    c, tr = make("tiny", dev, warmup=TRAJ_WARMUP)
    fx = load("latent_train_traj_tiny")
    w0 = grad_weights(c)
    losses, emas, lrs, _, _ = run_steps(tr, c, dev, 0, TRAJ_STEPS)
    for i in range(TRAJ_STEPS):
        assert lrs[i] == pytest.approx(float(fx["f64.lr"][i]), rel=1e-12), i
        assert float(losses[i]) == pytest.approx(float(fx["f64.loss"][i]), rel=1e-4), i
        assert rel_l2(emas[i], fx["f64.loss_ema"][i]) <= 1e-4, i
    worst = 0.0
    for k, q in tr.latent.named_parameters():
        ref = fx["f64.w." + k].double()
        w = q.detach().double().cpu()
        rms = lambda t: float(t.pow(2).mean().sqrt())
        tol = max(1e-5 * rms(ref) + 1e-3 * rms(ref - w0[k].double()) + 1e-7, 3 * float(fx["dist." + k]))
        assert rms(w - ref) <= tol, (k, rms(w - ref), tol)
        worst = max(worst, rms(w - ref) / tol)
    print(f"trajectory: final weights at {worst:.2e} of the tolerance")


def test_validation_epoch(dev):
    c, tr = make("tiny", dev)
    fx = load("latent_train_val_tiny")
    maps, ps = val_inputs(c)
    ema0 = tr.loss_ema.clone()
    tr.eval()
    tr.on_validation_epoch_start()
    for i, (m, p) in enumerate(zip(maps, ps)):
        tr.validation_step(on(m, dev), i, prior=p["prior"])
    logs = tr.on_validation_epoch_end()
    assert sorted(logs) == sorted(VAL_NAMES)
    for k, ref in zip(VAL_NAMES, fx["f64"].tolist()):
        print(f"{k}: {float(logs[k]):.7g} (reference {ref:.7g})")
        assert float(logs[k]) == pytest.approx(ref, rel=1e-4), k
    assert torch.equal(tr.loss_ema, ema0) and not bool(tr.loss_ema_initialized), "validation touched loss_ema"
    assert all(q.grad is None for q in tr.latent.parameters())


def test_state_dict_keys_and_round_trip(dev):
    fx = load("latent_train_val_tiny")
    det.force(True)
    try:
        c, tr = make("tiny", dev, warmup=TRAJ_WARMUP)
        sd = tr.state_dict()
        assert sorted(sd.keys()) == sorted(str(k) for k in fx["sd_keys"])
        assert sd["loss_ema_initialized"].dtype == torch.bool and sd["loss_ema"].shape == (11,)
        _, _, _, opt, sched = run_steps(tr, c, dev, 0, 2)
        assert tr.state_dict()["loss_ema_initialized"].dtype == torch.bool and bool(tr.loss_ema_initialized)
        saved = {k: v.clone() for k, v in tr.state_dict().items()}
        saved_opt, saved_sched = opt.state_dict(), sched.state_dict()
        import copy
        saved_opt = copy.deepcopy(saved_opt)
        want, want_ema, _, _, _ = run_steps(tr, c, dev, 2, 4, opt, sched)
        _, tr2 = make("tiny", dev, warmup=TRAJ_WARMUP)
        tr2.load_state_dict(saved)
        assert tr2.loss_ema_initialized.dtype == torch.bool and bool(tr2.loss_ema_initialized)
        tr2.gradient_clip_val = 1.0
        cfg = tr2.configure_optimizers()
        opt2, sched2 = cfg["optimizer"], cfg["lr_scheduler"]["scheduler"]
        opt2.load_state_dict(saved_opt)
        sched2.load_state_dict(saved_sched)
        got, got_ema, _, _, _ = run_steps(tr2, c, dev, 2, 4, opt2, sched2)
        for a, b in zip(want + want_ema, got + got_ema):
            assert torch.equal(a, b)
        for (k, a), (_, b) in zip(tr.latent.named_parameters(), tr2.latent.named_parameters()):
            assert torch.equal(a, b), k
    finally:
        det.force(None)


def test_eval_forward_is_bit_identical(dev):
    c, tr = make("tiny", dev)
    batch, p = on(train_batch(c, 11), dev), pins(c, 12)
    tr.eval()
    with torch.no_grad():
        a = tr(batch, prior=p["prior"])
        b = tr(batch, prior=p["prior"])
    assert torch.equal(a[0], b[0]) and all(torch.equal(a[1][k], b[1][k]) for k in LOG_NAMES)
    assert not a[0].requires_grad and not bool(tr.loss_ema_initialized)


@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["fp32", "bf16"])
def test_training_step_has_no_host_sync(mode):
    from osu_dreamer_amd import _lib
    _lib._lib = None
    _lib.lib()
    device = torch.device("cuda:0")
    c, tr = make("tiny", device, bf16=mode == "bf16")
    probe = torch.ones(1, device=device)
    torch.cuda.set_sync_debug_mode("error")
    try:
        try:
            probe.item()
            raised = False
        except RuntimeError:
            raised = True
    finally:
        torch.cuda.set_sync_debug_mode("default")
    if not raised:
        pytest.skip("this torch build does not raise on a synchronising .item() under set_sync_debug_mode('error')")
    tr.train()
    batches = [(on(b, device), {k: v.to(device) for k, v in p.items()}) for b, p in (traj_inputs(c, i) for i in range(3))]
    loss = tr(batches[0][0], **batches[0][1])          # the first step loads kernels and packs weights
    loss[0].backward()
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        for b, p in batches[1:]:
            for q in tr.latent.parameters():
                q.grad = None
            loss, _ = tr(b, **p)
            loss.backward()
    finally:
        torch.cuda.set_sync_debug_mode("default")
    torch.cuda.synchronize()
    assert bool(torch.isfinite(loss))
