"""bench.py quotes counter (`roofline.traffic`, `pmc_classes`) and sampler-parity records only when they were taken on the build it
runs: every record under profiles/ carries `kernel_src_sha` = od_build_source_sha() of the library that produced it."""
import json
import os

import pytest
import torch

from kernel_backend import dev  # noqa: F401


@pytest.fixture
def bench_mod(monkeypatch, tmp_path):
    import importlib
    import sys
    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    monkeypatch.syspath_prepend(repo)
    bench = importlib.import_module("bench")
    (tmp_path / "profiles").mkdir()
    monkeypatch.setattr(bench, "REPO", str(tmp_path))
    monkeypatch.setattr(bench, "_lib_sha", lambda: "aaaa000011112222")
    return bench, tmp_path / "profiles"


def test_traffic_record_needs_matching_build(bench_mod):
    bench, prof = bench_mod
    rec = {"B": 32, "L": 8192, "od_flash_attn_bwd": {"read_bytes": 10.0, "write_bytes": 5.0}, "classes": {"gemm_nt": {"mfma_busy": 0.4}}}
    (prof / "r02_traffic.json").write_text(json.dumps({**rec, "kernel_src_sha": "ffff"}))          # another build: never quoted
    traffic, classes, src = bench.load_pmc(32, 8192)
    assert traffic is None and classes is None and src["source"] is None and src["kernel_src_sha"] == "aaaa000011112222"
    (prof / "r03_traffic.json").write_text(json.dumps({**rec, "kernel_src_sha": "aaaa000011112222"}))
    traffic, classes, src = bench.load_pmc(32, 8192)
    assert traffic == 15 and classes == rec["classes"] and src["source"] == os.path.join("profiles", "r03_traffic.json")
    assert bench.load_pmc(8, 32768)[0] is None                                                   # another workload: not quoted either
    (prof / "r04_traffic.json").write_text("{ not json")                                          # a damaged newer record is skipped
    assert bench.load_pmc(32, 8192)[0] == 15


def test_sampler_parity_record_needs_matching_build(bench_mod):
    bench, prof = bench_mod
    modes = {"fp32": {"meets_1e-4": True, "rel_l2_vs_reference_fp32": 3e-7}}
    (prof / "r03_sampler_parity.json").write_text(json.dumps({"kernel_src_sha": "0123", "modes": modes}))
    assert bench.load_sampler_parity() == (None, None)
    (prof / "r03_sampler_parity.json").write_text(json.dumps({"kernel_src_sha": "aaaa000011112222", "modes": modes}))
    rec, src = bench.load_sampler_parity()
    assert rec["modes"] == modes and src.endswith("r03_sampler_parity.json")


def test_library_reports_its_source_hash():
    """od_build_source_sha(): 16 hex digits, and equal to what csrc/source_sha.sh computes from the tree the library was built from."""
    import subprocess
    from osu_dreamer_amd import _lib
    if not os.path.exists(_lib.DEFAULT_SO):
        pytest.skip("the HIP library has not been built")
    import ctypes
    cdll = ctypes.CDLL(_lib.DEFAULT_SO)
    cdll.od_build_source_sha.restype = ctypes.c_char_p
    sha = cdll.od_build_source_sha().decode()
    assert len(sha) == 16 and all(c in "0123456789abcdef" for c in sha)
    tree = subprocess.check_output(["bash", os.path.join(os.path.dirname(_lib.DEFAULT_SO), "csrc", "source_sha.sh")], text=True).strip()
    assert sha == tree, "the in-tree library is stale: run csrc/build.sh"


def test_power_sampler_energy(bench_mod, tmp_path):
    """joules_per_step: the hwmon energy counter's delta where the board has one, otherwise the 100 Hz power trace integrated over the timed
    region (trapezoid, the first / last reading held to the region's ends); None — never a made-up number — without readings."""
    bench, _ = bench_mod
    ps = bench.PowerSampler.__new__(bench.PowerSampler)
    ps.period, ps.dir = 0.01, None
    ps.samples, ps.times = [], []
    ps.t_enter, ps.t_exit, ps.e_enter, ps.e_exit = 10.0, 12.0, None, None
    assert ps.joules()[0] is None
    # a trace: 1000 W for the first second, ramping to 1400 W over the second one
    ps.times = [10.0 + 0.01 * i for i in range(1, 200)]
    ps.samples = [((1000.0 if t <= 11.0 else 1000.0 + 400.0 * (t - 11.0)), 2000.0) for t in ps.times]
    j, src = ps.joules()
    assert j == pytest.approx(1000.0 + 1200.0, rel=2e-3) and "integral" in src
    # an energy counter wins over the trace
    ps.e_enter, ps.e_exit = 5.0e6, 2.405e9
    j, src = ps.joules()
    assert j == pytest.approx(2400.0) and "energy1_input" in src
    # a hwmon directory without the files: every field None
    hw = tmp_path / "hwmon0"
    hw.mkdir()
    ps2 = bench.PowerSampler.__new__(bench.PowerSampler)
    ps2.dir = str(hw)
    assert ps2._num("energy1_input") is None and ps2._read() == (None, None)


def _tiny_bench_run(bench, device, steps, out_dir):
    """bench.py's timed path at toy widths (bench.synthetic_batch's channel counts, the tiny fixtures' backbone): the trainer seeded as
    make_trainer seeds it, `steps` steps of main()'s step(), then --dump-outputs.  Returns the trainer and the last step's loss."""
    from osu_dreamer_amd.lr_schedule import LRScheduleArgs
    from osu_dreamer_amd.model import BackboneArgs, DiffusionModelArgs
    from osu_dreamer_amd.train import DiffusionTrainer
    torch.manual_seed(1234)
    tr = DiffusionTrainer(val_batches=2, opt_args=dict(lr=3e-4, weight_decay=0.01),
                          schedule_args=LRScheduleArgs(warmup_init=.3, warmup_steps=1000, decay_start=30000),
                          osl_weight=1., del_weight=30., emb_dim=6, a_dim=128, style_dim=32,
                          diffusion_args=DiffusionModelArgs(global_cond_dim=32, backbone_dim=64, u_head_dim=16,
                                                            backbone_args=BackboneArgs(head_dim=32, n_heads=2, depth=2, expand=4, radius=2)))
    g = torch.Generator().manual_seed(1234)
    with torch.no_grad():
        for n, p in tr.diffusion.named_parameters():
            if any(z in n for z in ("ssg1.", "ssg2.", "proj_out.", "u_mod.")) or n == "u_out.weight":
                p.copy_(0.02 * torch.randn(p.shape, generator=g))
    tr.diffusion_ema.module.load_state_dict(tr.diffusion.state_dict())
    tr.gradient_clip_val = 1.0
    tr = tr.to(device)
    cfg = tr.configure_optimizers()
    opt, sched = cfg["optimizer"], cfg["lr_scheduler"]["scheduler"]
    batch = bench.synthetic_batch(2, 48, device, seed=1234)
    for i in range(steps):
        opt.zero_grad()
        loss = tr.training_step(batch, i)
        loss.backward()
        opt.step()
        sched.step()
        tr.on_train_batch_end()
    bench.dump_outputs(tr, str(out_dir))
    return tr, float(loss.detach())


def test_dump_outputs_holds_the_last_step(bench_mod, dev, tmp_path):
    """--dump-outputs: float32 / float64 .npy files, well under 64 MB, holding the last timed step's loss and the sampled weights,
    gradients and EMA weights at the positions sample_index.npy names; a second run with the same arguments writes the same arrays."""
    import numpy as np
    bench, _ = bench_mod
    tr, last_loss = _tiny_bench_run(bench, dev, 2, tmp_path / "a")
    files = sorted(os.listdir(tmp_path / "a"))
    assert files == sorted(f"{k}.npy" for k in ("loss", "osl", "del", "u_mape", "sample_index", "params", "grads", "ema_params"))
    arrs = {f[:-4]: np.load(tmp_path / "a" / f) for f in files}
    assert all(a.dtype in (np.float32, np.float64) for a in arrs.values())
    assert sum(os.path.getsize(tmp_path / "a" / f) for f in files) <= 64 << 20
    assert arrs["loss"].item() == pytest.approx(last_loss, rel=1e-6) and np.isfinite(arrs["loss"])
    named = list(tr.diffusion.named_parameters())
    ema = dict(tr.diffusion_ema.module.named_parameters())
    idx = arrs["sample_index"].astype(np.int64)
    total = sum(p.numel() for _, p in named)
    assert len(idx) == total and (np.diff(idx) > 0).all()          # toy model: fewer positions than DUMP_SAMPLE, so all of them
    flat = lambda ts: torch.cat([t.detach().reshape(-1).float().cpu() for t in ts]).numpy()[idx]
    np.testing.assert_array_equal(arrs["params"], flat([p for _, p in named]))
    np.testing.assert_array_equal(arrs["grads"], flat([p.grad for _, p in named]))
    np.testing.assert_array_equal(arrs["ema_params"], flat([ema[n] for n, _ in named]))
    assert np.abs(arrs["grads"]).max() > 0 and not np.array_equal(arrs["params"], arrs["ema_params"])
    _tiny_bench_run(bench, dev, 2, tmp_path / "b")
    for f in files:
        np.testing.assert_allclose(np.load(tmp_path / "b" / f), arrs[f[:-4]], rtol=1e-5, atol=1e-7, err_msg=f)
