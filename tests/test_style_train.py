"""Style-model training on the HIP path (osu_dreamer_amd/style_train.py) against the reference's own StyleTrainer
(osu_dreamer/models/style/train.py), recorded by tools/gen_style_train_golden.py into tests/golden/style_train_*.npz.

  * the two style-only backward kernels (od_style_conditioning_bwd, od_rmsnorm_rows_bwd) against fp64 autograd of the oracle's formulas;
  * one step: loss terms, every gradient tensor, the clip norm — fp32 (loss 1e-4, gradients rel-L2 1e-3, norm 2e-3; the reference itself
    sits ~1e-6 from its fp64 run on these inputs) and bf16 (test_model_parity's BF16_K rule: the reference's own bf16-vs-fp32 error per
    tensor is the yardstick);
  * 40 optimizer steps (clip 1.0, AdamW, warm-up / plateau / decay, EMA copy-then-lerp) under test_trajectory's rules;
  * one validation epoch: the four loss values, the K = 4 sample sets, the five sample metrics.

Every body runs on the emulator build (`-m "not gpu"`) and on the MI355X (`-m gpu`); the emulator skips h_dim > 64 as test_style.py does.
"""
import math
import os

import numpy as np
import pytest
import torch

from oracle import style_oracle as SO
from osu_dreamer_amd import ops
from osu_dreamer_amd.lr_schedule import LRScheduleArgs
from osu_dreamer_amd.style import StyleModel, StyleModelArgs
from osu_dreamer_amd.style_train import StyleTrainer, sample_metrics
from tools.gen_style_train_golden import (DEL_W, LABEL_DROP_PROB, LR, OSL_W, SUB, WEIGHT_DECAY, masks_every_column_both_ways, style_batch)
from kernel_backend import TOL, dev, rel_l2  # noqa: F401
from test_trajectory import check_weights

GOLDEN = os.path.join(os.path.dirname(__file__), "golden")
BF16_K, BF16_FLOOR = 3.0, 4e-3                   # tests/test_model_parity.py::run_bf16_training_case


def load(name):
    z = np.load(os.path.join(GOLDEN, name + ".npz"))
    return {k: (torch.from_numpy(np.asarray(z[k])) if z[k].dtype.kind != "U" else [str(s) for s in z[k]]) for k in z.files}


def dims_of(fx):
    v = [int(x) for x in fx["dims"].tolist()]
    return SO.StyleDims(style_dim=v[0], label_features=v[1], h_dim=v[2], depth=v[3], expand=v[4])


def make_trainer(d, P, device, warmup=10, decay_start=25):
    tr = StyleTrainer(opt_args=dict(lr=LR, weight_decay=WEIGHT_DECAY),
                      schedule_args=LRScheduleArgs(warmup_init=.3, warmup_steps=warmup, decay_start=decay_start),
                      label_drop_prob=LABEL_DROP_PROB, osl_weight=OSL_W, del_weight=DEL_W, style_dim=d.style_dim,
                      style_args=dict(label_features=d.label_features, h_dim=d.h_dim, depth=d.depth, expand=d.expand))
    tr.style.load_state_dict(P)
    tr.style_ema.module.load_state_dict(P)
    return tr.to(device)


def emu_skips_wide(dev, d):
    if dev.type == "cpu" and d.h_dim > 64:
        pytest.skip("wider style models run on the GPU only")


# ====================================================================================================== kernels against fp64 autograd
@pytest.mark.parametrize("B", [1, 7, 67])
def test_style_conditioning_bwd_against_fp64(dev, B):
    NL, F, H = 5, 16, 40
    g = torch.Generator().manual_seed(B)
    labels = torch.rand(B, NL, generator=g) * 10
    labels[torch.rand(B, NL, generator=g) < 0.3] = -1.0
    if B > 2:
        labels[0, :] = -1.0                          # a row with every label masked
        labels[1, :] = labels[1, :].abs() + 0.5      # a row with none masked
        labels[2, 1] = -float("inf")                 # a masked label whose Fourier features are NaN: a 0/1 multiply would leak them
    rw, rb = torch.randn(F, 1, generator=g) * 32, (torch.rand(F, generator=g) * 2 - 1) * math.pi
    dc = torch.randn(B, H, generator=g)
    init = [torch.randn(NL, F, H, generator=g), torch.randn(NL, H, generator=g), torch.randn(NL, H, generator=g)]   # the kernel accumulates
    P = {"rff.W": rw.double(), "rff.b": rb.double(), "cond_proj_w": torch.zeros(NL, F, H, dtype=torch.double, requires_grad=True),
         "cond_proj_b": torch.zeros(NL, H, dtype=torch.double, requires_grad=True),
         "null_labels": torch.zeros(NL, H, dtype=torch.double, requires_grad=True)}
    lab64 = torch.where(labels < 0, -1.0, labels).double()                                       # the oracle evaluates cos() for every label
    c = SO.conditioning(lab64, P, SO.StyleDims(label_features=F, h_dim=H))
    (c * dc.double()).sum().backward()
    outs = []
    for _ in range(2):
        got = [t.clone().to(dev) for t in init]
        ops.style_conditioning_bwd(labels.to(dev), rw.to(dev).contiguous(), rb.to(dev), dc.to(dev), *got)
        outs.append(got)
    for a, b in zip(*outs):
        assert torch.equal(a, b)                     # fixed summation order, no atomics
    for got, t0, k in zip(outs[0], init, ("cond_proj_w", "cond_proj_b", "null_labels")):
        assert torch.isfinite(got).all(), k
        ref = P[k].grad
        if float(ref.norm()) == 0:
            assert torch.equal(got.cpu(), t0), k
        else:
            assert rel_l2(got.cpu().double() - t0.double(), ref) < TOL[torch.float32], (k, B)


@pytest.mark.parametrize("accumulate", [False, True])
@pytest.mark.parametrize("gamma_on", [False, True])
@pytest.mark.parametrize("M,C", [(1, 32), (5, 40), (131, 256)])
def test_rmsnorm_rows_bwd_against_fp64(dev, M, C, gamma_on, accumulate):
    g = torch.Generator().manual_seed(M * 1000 + C)
    x, dy = torch.randn(M, C, generator=g) * 1.7, torch.randn(M, C, generator=g)
    gamma = 1 + 0.3 * torch.randn(C, generator=g) if gamma_on else None
    eps = float(torch.finfo(torch.float32).eps) if gamma_on else 1e-6
    dx0, dg0 = torch.randn(M, C, generator=g), torch.randn(C, generator=g)
    x64 = x.double().requires_grad_(True)
    g64 = gamma.double().requires_grad_(True) if gamma_on else None
    y = SO.rms_rows(x64, eps)
    if gamma_on:
        y = y * g64
    (y * dy.double()).sum().backward()
    outs = []
    for _ in range(2):
        dx, dg = dx0.clone().to(dev), dg0.clone().to(dev)
        ops.rmsnorm_rows_bwd(x.to(dev), None if gamma is None else gamma.to(dev), dy.to(dev), dx, dg if gamma_on else None, eps, accumulate)
        outs.append((dx, dg))
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])
    dx, dg = outs[0]
    base = dx0.double() if accumulate else torch.zeros(M, C, dtype=torch.double)
    assert rel_l2(dx.cpu().double() - base, x64.grad) < TOL[torch.float32]
    if gamma_on:
        assert rel_l2(dg.cpu().double() - dg0.double(), g64.grad) < TOL[torch.float32]
    else:
        assert torch.equal(dg.cpu(), dg0)            # untouched
    # the forward it differentiates
    yk = torch.empty(M, C, device=dev)
    ops.rmsnorm_rows(x.to(dev), None if gamma is None else gamma.to(dev), yk, eps)
    assert rel_l2(yk, y) < TOL[torch.float32]


# ====================================================================================================== one step against the reference
def run_step(name, dev, tag, gemm_min_rows=None):
    fx = load(name)
    d = dims_of(fx)
    emu_skips_wide(dev, d)
    B = int(fx["B"])
    batch = style_batch(d, B, int(fx["batch_seed"]))
    for k, v in batch.items():
        assert torch.equal(v, fx["in." + k]), k                    # the fixture's recorded draws are the seed's
    assert masks_every_column_both_ways(batch["drop"])
    P = SO.init_style_params(d, int(fx["seed"]))
    tr = make_trainer(d, P, dev)
    model = tr.style
    model.compute_dtype = torch.bfloat16 if tag == "bf16" else torch.float32
    if gemm_min_rows is not None:
        model.gemm_min_rows = gemm_min_rows
    opt = tr.configure_optimizers()["optimizer"]
    opt.zero_grad()
    loss, logs = tr(model, None, None, batch["s1"].to(dev), batch["labels"].to(dev), t=batch["t"].to(dev), s0=batch["s0"].to(dev),
                    drop=batch["drop"].to(dev))
    loss.backward()
    grads = {k: p.grad.detach().cpu() for k, p in model.named_parameters()}
    assert sorted(grads) == sorted(k for k in P if not k.startswith("rff."))
    gn = float(model.arena.grad.double().norm())
    whole = "f32.grad.proj_in.weight" in fx
    pick = (lambda g: g) if whole else (lambda g: g.flatten()[::max(1, g.numel() // SUB)][:SUB])
    kind = "grad" if whole else "gradsub"
    worst = 0.0
    if tag == "f32":
        for k in ("loss", "osl", "del", "u_mape"):
            print(f"[{name}/f32] {k}: {float(logs[k]):.7f} (ref {float(fx['f32.' + k]):.7f})")
            assert float(logs[k]) == pytest.approx(float(fx["f32." + k]), rel=1e-4), k
        print(f"[{name}/f32] clip norm {gn:.6f} (ref {float(fx['f32.grad_norm']):.6f})")
        assert gn == pytest.approx(float(fx["f32.grad_norm"]), rel=2e-3)
        for k, g in grads.items():
            e = rel_l2(pick(g), fx[f"f32.{kind}.{k}"])
            worst = max(worst, e)
            assert e <= 1e-3, (k, e)
            assert float(g.norm()) == pytest.approx(float(fx["f32.gradnorm." + k]), rel=1e-3), k
        print(f"[{name}/f32] worst gradient rel-L2 {worst:.3e}")
    else:
        for k in ("loss", "osl", "del"):
            r32, r16 = float(fx["f32." + k]), float(fx["bf16." + k])
            print(f"[{name}/bf16] {k}: {float(logs[k]):.6f} (ref fp32 {r32:.6f}, ref bf16 {r16:.6f})")
            assert abs(float(logs[k]) - r32) <= BF16_K * abs(r16 - r32) + 2e-3 * abs(r32), (k, float(logs[k]), r32, r16)
        gn32, gn16 = float(fx["f32.grad_norm"]), float(fx["bf16.grad_norm"])
        print(f"[{name}/bf16] clip norm {gn:.6f} (ref fp32 {gn32:.6f}, ref bf16 {gn16:.6f})")
        assert abs(gn - gn32) <= BF16_K * abs(gn16 - gn32) + 5e-3 * gn32, (gn, gn32, gn16)
        for k, g in grads.items():
            r32, r16 = fx[f"f32.{kind}.{k}"], fx[f"bf16.{kind}.{k}"]
            n32 = float(fx["f32.gradnorm." + k])
            assert abs(float(g.norm()) - n32) <= BF16_K * abs(float(fx["bf16.gradnorm." + k]) - n32) + 2e-2 * n32 + 1e-7, k
            e_ref, e_mine = rel_l2(r16, r32), rel_l2(pick(g), r32)
            assert e_mine <= BF16_K * e_ref + BF16_FLOOR, (k, e_mine, e_ref)
            worst = max(worst, e_mine / max(e_ref, 1e-9))
        print(f"[{name}/bf16] worst gradient distance = {worst:.2f} x the reference's own bf16 error")


@pytest.mark.parametrize("tag", ["f32", "bf16"])
@pytest.mark.parametrize("name", ["style_train_step_tiny", "style_train_step_mid", "style_train_step_full"])
def test_step_against_reference(dev, name, tag):
    run_step(name, dev, tag)


@pytest.mark.parametrize("tag", ["f32", "bf16"])
@pytest.mark.parametrize("min_rows", [1, 10 ** 6])
def test_step_on_either_product_route(dev, tag, min_rows):
    """The fp32 products go through od_linear_small below `gemm_min_rows` batch rows and through the fp32 MFMA GEMMs from there on: the
    tiny step under both routes (the mid and full fixtures above take the routes their batch sizes select: 48 and 512 rows)."""
    run_step("style_train_step_tiny", dev, tag, gemm_min_rows=min_rows)


@pytest.mark.gpu
@pytest.mark.parametrize("min_rows", [1, 10 ** 6])
def test_full_step_on_either_product_route(min_rows):
    from osu_dreamer_amd import _lib
    _lib._lib = None
    _lib.lib()
    run_step("style_train_step_full", torch.device("cuda:0"), "f32", gemm_min_rows=min_rows)


def test_fixture_reference_is_close_to_fp64():
    """The bounds above can neither be met by accident nor missed by the reference: its fp32 gradients are ~1e-6 from its fp64 run."""
    for name in ("style_train_step_tiny", "style_train_step_mid", "style_train_step_full"):
        fx = load(name)
        assert float(fx["f32_vs_f64_worst"]) < 1e-5
        assert float(fx["f32.loss"]) == pytest.approx(float(fx["f64.loss"]), rel=1e-5)


def test_inference_copies_stay_frozen_and_trainer_model_trains(dev):
    d = SO.STYLE_TINY
    m = StyleModel(d.style_dim, StyleModelArgs(d.label_features, d.h_dim, d.depth, d.expand))
    assert not any(p.requires_grad for p in m.parameters())
    tr = make_trainer(d, SO.init_style_params(d, 1), dev)
    assert all(p.requires_grad for p in tr.style.parameters())
    assert not any(p.requires_grad for p in tr.style_ema.module.parameters())
    assert set(dict(tr.style.named_buffers())) == {"rff.W", "rff.b"}
    assert all(p.data_ptr() >= tr.style.arena.data.data_ptr() for p in tr.style.parameters())
    opt = tr.configure_optimizers()["optimizer"]
    assert {id(p) for g in opt.param_groups for p in g["params"]} == {id(p) for p in tr.style.parameters()}      # train.py:94


def test_dropout_in_training_mode_raises(dev):
    d = SO.STYLE_TINY
    tr = StyleTrainer(opt_args=dict(lr=LR), schedule_args=LRScheduleArgs(), label_drop_prob=.2, osl_weight=1., del_weight=30.,
                      style_dim=d.style_dim, style_args=dict(label_features=d.label_features, h_dim=d.h_dim, depth=d.depth,
                                                             expand=d.expand, dropout=0.1)).to(dev)
    b = style_batch(d, 4, 5)
    tr.train()
    with pytest.raises(NotImplementedError, match="model.py:67"):
        tr(tr.style, None, None, b["s1"].to(dev), b["labels"].to(dev))


# ====================================================================================================== 40-step trajectory
def run_trajectory(name, device, tag, steps):
    fx = load(name)
    d = dims_of(fx)
    total, B = int(fx["steps"]), int(fx["B"])
    steps = min(steps, total)
    P0 = SO.init_style_params(d, int(fx["seed"]))
    tr = make_trainer(d, P0, device, warmup=int(fx["warmup_steps"]), decay_start=int(fx["decay_start"]))
    model = tr.style
    model.compute_dtype = torch.bfloat16 if tag == "bf16" else torch.float32
    tr.gradient_clip_val = 1.0
    cfg = tr.configure_optimizers()
    opt, sched = cfg["optimizer"], cfg["lr_scheduler"]["scheduler"]
    assert opt.max_grad_norm == 1.0
    worst = 0.0
    for i in range(steps):
        b = {k: v.to(device) for k, v in style_batch(d, B, int(fx["batch_seed"]) + i).items()}
        assert opt.param_groups[0]["lr"] == pytest.approx(float(fx[f"{tag}.lr"][i]), rel=1e-9), i
        opt.zero_grad()
        loss = tr.training_step((None, None, b["s1"], b["labels"]), i, t=b["t"], s0=b["s0"], drop=b["drop"])
        loss.backward()
        opt.step()
        sched.step()
        tr.on_train_batch_end()
        mine, ref = float(loss.detach()), float(fx[f"{tag}.loss"][i])
        gn, gref = float(opt.gnorm_sq.sqrt()), float(fx[f"{tag}.grad_norm"][i])
        if tag == "f32":
            assert mine == pytest.approx(ref, rel=1e-4), (i, mine, ref)
            assert gn == pytest.approx(gref, rel=2e-3), (i, gn, gref)
            worst = max(worst, abs(mine - ref) / abs(ref))
        else:
            ref32 = float(fx["f32.loss"][i])
            bound = 3.0 * abs(ref - ref32) + 2e-3 * abs(ref32)
            assert abs(mine - ref) <= bound, (i, mine, ref, ref32)
            worst = max(worst, abs(mine - ref) / bound)
    assert int(tr.style_ema.n_averaged) == steps
    assert "train/loss" in tr._logged and "train/u_mape" in tr._logged
    if steps == total:
        assert int(tr.style_ema.n_averaged) == int(fx[f"{tag}.n_averaged"])
        weights = {k: p.detach().cpu() for k, p in model.named_parameters()}
        ema = {k: p.detach().cpu() for k, p in tr.style_ema.module.named_parameters()}
        ww = check_weights(fx, tag, P0, weights, ema, k_drift=3.0 if tag == "bf16" else 0.0, label="hip style")
        print(f"[{name}/{tag}] {steps} steps: worst loss error {worst:.3e} ({'relative' if tag == 'f32' else 'of its bound'}), "
              f"final weights at {ww:.2e} of the tolerance")


@pytest.mark.parametrize("tag", ["f32", "bf16"])
def test_trajectory_prefix_tiny(dev, tag):
    run_trajectory("style_train_traj40_tiny", dev, tag, 10)


@pytest.mark.gpu
@pytest.mark.parametrize("tag", ["f32", "bf16"])
@pytest.mark.parametrize("name", ["style_train_traj40_tiny", "style_train_traj40_mid"])
def test_trajectory_40_steps(name, tag):
    from osu_dreamer_amd import _lib
    _lib._lib = None
    _lib.lib()
    run_trajectory(name, torch.device("cuda:0"), tag, 40)


# ====================================================================================================== one validation epoch
def test_validation_epoch(dev):
    fx = load("style_train_val_tiny")
    d = dims_of(fx)
    B, K = int(fx["B"]), int(fx["K"])
    P = SO.init_style_params(d, int(fx["seed"]))
    tr = make_trainer(d, P, dev)
    b = {k[3:]: v.to(dev) for k, v in fx.items() if k.startswith("in.")}
    taken = []
    real = tr.style_ema.module.sample

    def sample(labels, n, s_init=None):
        assert n == 16
        out = real(labels, n, s_init=s_init)
        taken.append(out.detach().cpu())
        return out
    tr.style_ema.module.sample = sample
    tr.on_validation_epoch_start()
    h = B // 2
    for i, sl in enumerate((slice(0, h), slice(h, B))):
        tr.validation_step((None, None, b["s1"][sl], b["labels"][sl]), i)
    logs = tr.on_validation_epoch_end(t=b["t"], s0=b["s0"], drop=b["drop"], s_init=[s.to(dev) for s in fx["s_init"]])
    names = ["val/loss", "val/osl", "val/del", "val/u_mape", "val/nn_ratio", "val/nn_ratio_sr5", "val/cond_recall", "val/sample_spread",
             "val/energy_dist"]
    assert sorted(logs) == sorted(names) and all(k in tr._logged for k in names)
    for k in names[:4]:
        print(f"[val] {k}: {float(logs[k]):.7f} (ref {float(fx['f32.' + k]):.7f})")
        assert float(logs[k]) == pytest.approx(float(fx["f32." + k]), rel=1e-4), k
    assert len(taken) == K
    for k in range(K):
        assert rel_l2(taken[k], fx["samples"][k]) < 1e-4, k
    for k in names[4:]:
        print(f"[val] {k}: {float(logs[k]):.7f} (ref fp32 {float(fx['f32.' + k]):.7f}, fp64 {float(fx['f64.' + k]):.7f})")
        assert float(logs[k]) == pytest.approx(float(fx["f32." + k]), rel=1e-3), k
        assert float(fx["f32." + k]) == pytest.approx(float(fx["f64." + k]), rel=1e-4), k
    # the metric code itself, on the fixture's own samples in fp64
    for k, v in sample_metrics(fx["samples"].double(), b["s1"].cpu().double(), b["labels"].cpu().double()).items():
        assert float(v) == pytest.approx(float(fx["f64." + k]), rel=1e-9), k


def test_state_dict_layout_and_hparams(dev):
    fx = load("style_train_val_tiny")
    d = dims_of(fx)
    tr = make_trainer(d, SO.init_style_params(d, 1), dev)
    assert sorted(tr.state_dict().keys()) == sorted(fx["sd_keys"])               # the reference StyleTrainer's key set
    hp = tr.hparams_dict
    assert hp["style_dim"] == d.style_dim and isinstance(hp["style_args"], dict) and hp["style_args"]["h_dim"] == d.h_dim
    # a round trip through state_dict keeps the weights, the average and its count
    tr.style_ema.update_parameters(tr.style)
    tr2 = make_trainer(d, SO.init_style_params(d, 2), dev)
    tr2.load_state_dict(tr.state_dict())
    assert int(tr2.style_ema.n_averaged) == 1 and tr2.style_ema.count == 1
    for (k, a), (_, b) in zip(tr.state_dict().items(), tr2.state_dict().items()):
        assert torch.equal(a, b), k


# ====================================================================================================== deterministic mode, captured graph
def one_step(tr, d, B, seed, device):
    b = {k: v.to(device) for k, v in style_batch(d, B, seed).items()}
    opt = tr.configure_optimizers()["optimizer"]
    opt.zero_grad()
    loss, logs = tr(tr.style, None, None, b["s1"], b["labels"], t=b["t"], s0=b["s0"], drop=b["drop"])
    loss.backward()
    return {k: float(v) for k, v in logs.items()}, tr.style.arena.grad.detach().clone()


def test_deterministic_mode_repeats_bit_for_bit(dev):
    """OD_DETERMINISTIC: the step's atomically accumulated sums (od_linear_small_bwd's dx slices, the u-head's weight gradient, the loss
    scalars) go through integer shadows: two steps from the same state are bit-identical, and within fp32 rounding of the plain step."""
    from osu_dreamer_amd import det
    d, B = SO.STYLE_TINY, 9
    P = SO.init_style_params(d, 4)
    plain_logs, plain = one_step(make_trainer(d, P, dev), d, B, 77, dev)
    det.force(True)
    try:
        runs = [one_step(make_trainer(d, P, dev), d, B, 77, dev) for _ in range(2)]
    finally:
        det.force(None)
    assert runs[0][0] == runs[1][0] and torch.equal(runs[0][1], runs[1][1])
    assert rel_l2(runs[0][1], plain) < TOL[torch.float32]
    assert runs[0][0]["loss"] == pytest.approx(plain_logs["loss"], rel=1e-6)


_DET_CHILD = """
import sys, torch
sys.path.insert(0, {repo!r}); sys.path.insert(0, {tests!r})
from oracle import style_oracle as SO
from test_style_train import make_trainer, one_step
from tools.gen_style_train_golden import STYLE_MID
dev = torch.device("cuda:0")
P = SO.init_style_params(STYLE_MID, 5)
out = []
for use_graph in (False, True, True):
    tr = make_trainer(STYLE_MID, P, dev)
    tr.use_graph = use_graph
    out.append(one_step(tr, STYLE_MID, 48, 9, dev))
    assert tr._graph.captures == int(use_graph)
for logs, g in out[1:]:
    assert logs == out[0][0], (logs, out[0][0])
    assert torch.equal(g, out[0][1])
print("DET-EQUAL")
"""


@pytest.mark.gpu
@pytest.mark.parametrize("tag", ["f32", "bf16"])
def test_captured_step_matches_eager(tag):
    from osu_dreamer_amd import _lib
    from tools.gen_style_train_golden import STYLE_MID
    _lib._lib = None
    _lib.lib()
    device = torch.device("cuda:0")
    d, B = STYLE_MID, 48
    P = SO.init_style_params(d, 5)
    res = {}
    for use_graph in (False, True):
        tr = make_trainer(d, P, device)
        tr.style.compute_dtype = torch.bfloat16 if tag == "bf16" else torch.float32
        tr.use_graph = use_graph
        res[use_graph] = (tr, *one_step(tr, d, B, 9, device))
        assert tr._graph.captures == int(use_graph)
    (_, logs_e, g_e), (trg, logs_g, g_g) = res[False], res[True]
    assert logs_g == logs_e                                              # the forward and the loss have no atomics at these sizes
    for k in trg.style.arena.entries:
        a, b = trg.style.arena.view(k, g_g), trg.style.arena.view(k, g_e)
        assert rel_l2(a, b) < TOL[torch.float32], k                      # weight gradients meet in fp32 atomics
    # same shape, new inputs: replays the captured graph, and computes what an eager step computes on them
    logs2, g2 = one_step(trg, d, B, 10, device)
    assert trg._graph.captures == 1
    tre = make_trainer(d, P, device)
    tre.style.compute_dtype, tre.use_graph = trg.style.compute_dtype, False
    logs2e, g2e = one_step(tre, d, B, 10, device)
    assert logs2 == logs2e and rel_l2(g2, g2e) < TOL[torch.float32]
    assert logs2 != logs_g
    # another batch size: a new capture
    one_step(trg, d, B // 2, 11, device)
    assert trg._graph.captures == 2


@pytest.mark.gpu
def test_captured_step_is_bit_identical_in_deterministic_mode():
    import subprocess
    import sys
    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, OD_DETERMINISTIC="1")
    r = subprocess.run([sys.executable, "-c", _DET_CHILD.format(repo=repo, tests=os.path.join(repo, "tests"))], env=env, capture_output=True,
                       text=True, timeout=300)
    assert r.returncode == 0 and "DET-EQUAL" in r.stdout, r.stdout + r.stderr
