"""The denoiser with head_dim 128 end to end, against fixtures the REFERENCE produced with that head dim (tools/gen_hd128_golden.py; weights
and batches regenerated from the seed on both sides), under test_model_parity.py's own `run_case` / `run_bf16_training_case` and bounds:
forward, bf16 forward, sampler (eager and graph), fp32-as-3-x-bf16, loss, every gradient, two optimizer + EMA steps, and the bf16 step.

  tiny_hd128_b2_l130 / train_bf16_tiny_hd128_b2_l130   backbone 64, 2 heads x 128, depth 2, B 2 x L 130 (three key tiles, the last ragged;
                                                        two query workgroups, the second ragged) — emulator and GPU
  full_hd128_d2_b2_l96                                  backbone 512 as 4 heads x 128, depth 2 — GPU only
plus forward(..., lengths=) on two songs of different length against each song alone, as test_sample_many.py holds head_dim 64, and a
`fit-denoiser` run from a config with head_dim 128 whose checkpoint loads back.
"""
import pytest
import torch
import yaml

from osu_dreamer_amd.model import DiffusionModel
from oracle import denoiser_oracle as O
from kernel_backend import dev  # noqa: F401
from test_model_parity import margs, run_bf16_training_case, run_case
from test_sampler50 import rel
from tools.gen_hd128_golden import CASES, TINY_HD128


def test_tiny_hd128_vs_reference(dev):
    run_case("tiny_hd128_b2_l130", dev)


def test_bf16_training_step_tiny_hd128(dev):
    run_bf16_training_case("train_bf16_tiny_hd128_b2_l130", dev)


@pytest.mark.gpu
def test_full_width_hd128_vs_reference():
    from osu_dreamer_amd import _lib
    _lib._lib = None
    _lib.lib()
    assert CASES["full_hd128_d2_b2_l96"][1].head_dim == 128 and CASES["full_hd128_d2_b2_l96"][1].backbone_dim == 512
    run_case("full_hd128_d2_b2_l96", torch.device("cuda:0"))


def _model(dev):
    d = TINY_HD128
    m = DiffusionModel(d.emb_dim, d.a_dim, d.style_dim, margs(d))
    m.load_state_dict(O.init_params(d, seed=2100))
    return m.to(dev).eval()


def _song(m, L, B, seed, dev):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(1, m.a_dim, L, generator=g).to(dev), torch.randn(B, m.style_dim, generator=g).to(dev),
            torch.randn(B, m.emb_dim, L, generator=g).to(dev))


MODES = (("fp32", None, "f32"), ("fp32_bf16x3", None, "bf16x3"), ("bf16", torch.bfloat16, "f32"))


@pytest.mark.parametrize("mode,dt,mm", MODES, ids=[x[0] for x in MODES])
def test_forward_lengths_matches_each_song_alone_hd128(dev, mode, dt, mm):
    """Two songs, 70 and 150 frames (padded to 192: the short one ends inside the second key tile and leaves a whole padded query tile),
    in one varlen forward against each alone.  Bounds as test_sample_many.py: 1e-5 in fp32 / x3, 1e-3 in bf16."""
    m = _model(dev)
    m.compute_dtype, m.f32_matmul = dt, mm
    songs = [_song(m, L, B, 100 + i, dev) for i, (L, B) in enumerate(((70, 2), (150, 1)))]
    Lpad = 192
    Bt = sum(s[1].shape[0] for s in songs)
    audio = torch.zeros(Bt, m.a_dim, Lpad, device=dev)
    xt = torch.zeros(Bt, m.emb_dim, Lpad, device=dev)
    lengths, r = [], 0
    for a, s, x in songs:
        n, L = s.shape[0], a.shape[-1]
        audio[r:r + n, :, :L] = a[0]
        xt[r:r + n, :, :L] = x
        lengths += [L] * n
        r += n
    style = torch.cat([s[1] for s in songs])
    bound = 1e-3 if mode == "bf16" else 1e-5
    with torch.no_grad():
        u, v = m(audio, style, xt, lengths=lengths)
        r = 0
        for a, s, x in songs:
            n, L = s.shape[0], a.shape[-1]
            u1, v1 = m(a, s, x)
            assert rel(u[r:r + n], u1) <= bound, (mode, L, rel(u[r:r + n], u1))
            assert rel(v[r:r + n, :, :L], v1) <= bound, (mode, L, rel(v[r:r + n, :, :L], v1))
            assert torch.count_nonzero(v[r:r + n, :, L:]).item() == 0
            r += n


def test_sample_many_hd128_matches_sample(dev):
    """sample_many on the same two songs against sample() on each alone, fp32, 6 steps.  Each side is a sampler run the fixture test above
    holds within 1e-4 relative L2 of the reference's; two such runs are within 2e-4 of each other."""
    m = _model(dev)
    songs = [_song(m, L, B, 200 + i, dev) for i, (L, B) in enumerate(((70, 2), (150, 1)))]
    outs = m.sample_many([s[0] for s in songs], [s[1] for s in songs], 6, x_init=[s[2] for s in songs])
    for (a, s, x), out in zip(songs, outs):
        assert tuple(out.shape) == tuple(x.shape) and bool(torch.isfinite(out).all())
        alone = m.sample(a, s, 6, x_init=x)
        assert rel(out, alone) <= 2e-4, (a.shape[-1], rel(out, alone))


def test_fit_denoiser_hd128(dev, tmp_path):
    """`fit-denoiser` from a config with head_dim: 128, n_heads: 4 (the tiny test config otherwise): three steps, one validation, and a
    checkpoint whose hyper-parameters and EMA weights build a DiffusionModel that runs."""
    from osu_dreamer_amd.data import LatentDataModule, write_synthetic_dataset
    from osu_dreamer_amd.fit import DEFAULT_CONFIG, build_from_config
    cfg = yaml.safe_load(open(DEFAULT_CONFIG))
    cfg["model"].update(emb_dim=6, a_dim=16, style_dim=8)
    cfg["model"]["diffusion_args"] = dict(global_cond_dim=32, u_head_dim=16, backbone_dim=64,
                                          backbone_args=dict(head_dim=128, n_heads=4, depth=2, expand=2, radius=1))
    data_dir = tmp_path / "data"
    write_synthetic_dataset(str(data_dir), n_maps=4, frames=160, a_dim=16, emb_dim=6, style_dim=8, seed=1)
    cfg["data"].update(data_path=str(data_dir), seq_len=130, batch_size=2, num_workers=0, shuffle_buffer_size=1, max_val_count=128,
                       max_per_map=-1)
    cfg["trainer"].update(max_steps=3, log_every_n_steps=1, val_check_interval=3, limit_val_batches=1, default_root_dir=str(tmp_path / "run"),
                          precision="32" if dev.type == "cpu" else "bf16-mixed")
    torch.manual_seed(0)
    module, trainer = build_from_config(cfg)
    with torch.no_grad():
        for n, p in module.diffusion.named_parameters():
            if any(z in n for z in ("ssg1.", "ssg2.", "proj_out.", "u_mod.")):
                p.normal_(0, 0.02)
    hist = trainer.fit(module, LatentDataModule(**cfg["data"]))
    train = [h for h in hist if "train/loss" in h]
    assert len(train) == 3 and all(torch.isfinite(torch.tensor(h["train/loss"])) for h in train)
    assert [h["val/loss"] > 0 for h in hist if "val/loss" in h] == [True]
    ck = torch.load(tmp_path / "run" / "checkpoints" / "best.ckpt", map_location="cpu", weights_only=False)
    ba = ck["hyper_parameters"]["diffusion_args"]["backbone_args"]
    assert ba["head_dim"] == 128 and ba["n_heads"] == 4
    m = DiffusionModel(6, 16, 8, margs(O.Dims(emb_dim=6, a_dim=16, style_dim=8, global_cond_dim=32, backbone_dim=64, n_heads=4, head_dim=128,
                                              depth=2, expand=2, radius=1, u_head_dim=16)))
    m.load_state_dict({k.removeprefix("diffusion_ema.module."): v for k, v in ck["state_dict"].items() if k.startswith("diffusion_ema.module.")})
    m = m.to(dev).eval()
    a, s, x = _song(m, 100, 2, 5, dev)
    xs = m.sample(a, s, 3, x_init=x)
    assert tuple(xs.shape) == (2, 6, 100) and bool(torch.isfinite(xs).all())
