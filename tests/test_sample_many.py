"""DiffusionModel.forward(..., lengths=) and DiffusionModel.sample_many on the 46.9 M-parameter model of tests/golden/sample50_full_d8_b4_l1115.npz
(built the way test_sampler50.py builds it): several songs of different lengths in one batched call, zero-padded to a common length, each song
held to its own frames and its own sampler step size.
  1. one forward with `lengths` against `forward` on each song alone;
  2. the fixture's song inside two mixed batches (padded, and the longest) against the reference's own 50-step run;
  3. one song whose length is a multiple of 64 (no padding): sample_many == sample(), bit for bit under OD_DETERMINISTIC;
  4. two calls with other lengths but the same (B, Lpad) replay one captured graph, bit for bit an uncaptured run (OD_DETERMINISTIC).
"""
import pytest
import torch

from osu_dreamer_amd import det
from test_sampler50 import BOUND, load, problem, rel

pytestmark = pytest.mark.gpu

MODES = (("fp32", None, "f32"), ("fp32_bf16x3", None, "bf16x3"), ("bf16", torch.bfloat16, "f32"))


@pytest.fixture(scope="module")
def setup():
    from osu_dreamer_amd import _lib
    from osu_dreamer_amd.model import BackboneArgs, DiffusionModel, DiffusionModelArgs
    _lib.lib()
    dev = torch.device("cuda:0")
    fx = load("sample50_full_d8_b4_l1115")
    d, P, data = problem(fx)
    m = DiffusionModel(d.emb_dim, d.a_dim, d.style_dim,
                       DiffusionModelArgs(d.global_cond_dim, d.backbone_dim,
                                          BackboneArgs(d.depth, d.expand, d.head_dim, d.n_heads, d.radius), d.u_head_dim))
    m.load_state_dict(P)
    m = m.to(dev).eval()
    yield m, fx, data, dev
    m.compute_dtype, m.f32_matmul, m.use_graph = None, "f32", True


def _set_mode(m, dt, mm):
    m.compute_dtype, m.f32_matmul = dt, mm


def _song(m, L, B, seed, dev):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(1, m.a_dim, L, generator=g).to(dev), torch.randn(B, m.style_dim, generator=g).to(dev),
            torch.randn(B, m.emb_dim, L, generator=g).to(dev))


@pytest.mark.parametrize("mode,dt,mm", MODES, ids=[x[0] for x in MODES])
def test_forward_lengths_matches_each_song_alone(setup, mode, dt, mm):
    m, _, _, dev = setup
    _set_mode(m, dt, mm)
    songs = [_song(m, L, B, 100 + i, dev) for i, (L, B) in enumerate(((700, 2), (1115, 4), (1500, 3)))]
    Lpad = (1500 + 63) // 64 * 64
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
    with torch.no_grad():
        u, v = m(audio, style, xt, lengths=lengths)
        torch.cuda.synchronize()
        bound = 1e-3 if mode == "bf16" else 1e-5
        r = 0
        for a, s, x in songs:
            n, L = s.shape[0], a.shape[-1]
            u1, v1 = m(a, s, x)
            assert rel(u[r:r + n], u1) <= bound, (mode, L, rel(u[r:r + n], u1))
            assert rel(v[r:r + n, :, :L], v1) <= bound, (mode, L, rel(v[r:r + n, :, :L], v1))
            assert torch.count_nonzero(v[r:r + n, :, L:]).item() == 0
            r += n
    with pytest.raises(RuntimeError):           # no varlen backward
        with torch.enable_grad():
            m(audio, style, xt, lengths=lengths)


@pytest.mark.parametrize("mode,dt,mm", MODES, ids=[x[0] for x in MODES])
def test_sample_many_fixture_song_vs_reference(setup, mode, dt, mm):
    m, fx, data, dev = setup
    _set_mode(m, dt, mm)
    h, s, x_init = data["h"].to(dev), data["s"].to(dev), data["x_init"].to(dev)
    steps = int(fx["num_steps"])
    ref, ref_bf16 = fx["sample_x"], fx["sample_x_bf16"]
    for other_L, other_B, first in ((1500, 2, True), (400, 3, False)):      # the fixture's song padded (to 1536), then the longest (1152)
        a2, s2, x2 = _song(m, other_L, other_B, 7, dev)
        if first:
            outs = m.sample_many([h, a2], [s, s2], steps, x_init=[x_init, x2])
            xs, g = outs[0], 0
        else:
            outs = m.sample_many([a2, h], [s2, s], steps, x_init=[x2, x_init])
            xs, g = outs[1], 1
        torch.cuda.synchronize()
        assert all(torch.isfinite(o).all() for o in outs)
        assert tuple(outs[1 - g].shape) == (other_B, m.emb_dim, other_L)
        e = rel(xs, ref)
        eta = m.last_sample_stats
        assert tuple(eta.shape) == (2, 2)
        if mode == "bf16":
            assert e < 3 * rel(ref_bf16, ref) + 1e-3, (mode, other_L, e)
        else:
            assert e < BOUND, (mode, other_L, e)
            assert abs(float(eta[g, 0]) - float(fx["eta"])) < 1e-5 * abs(float(fx["eta"])) + 1e-7


def test_sample_many_one_song_without_padding_equals_sample(setup):
    m, fx, data, dev = setup
    _set_mode(m, None, "f32")
    L = 1088                                            # a multiple of 64: Lpad = L
    h, s, x_init = data["h"][..., :L].to(dev), data["s"].to(dev), data["x_init"][..., :L].to(dev)
    try:
        det.force(True)
        a = m.sample(h, s, 8, x_init=x_init)
        eta_a = m.last_sample_stats.clone()
        b = m.sample_many([h], [s], 8, x_init=[x_init])[0]
        assert torch.equal(a, b)
        assert torch.equal(eta_a, m.last_sample_stats[0])
    finally:
        det.force(None)
    a = m.sample(h, s, 8, x_init=x_init)
    b = m.sample_many([h], [s], 8, x_init=[x_init])[0]
    assert rel(b, a) <= 1e-6


def test_sample_many_reuses_the_graph_across_lengths(setup):
    m, _, _, dev = setup
    _set_mode(m, None, "f32")
    calls = [[_song(m, 1000, 2, 11, dev), _song(m, 700, 3, 12, dev)], [_song(m, 1020, 2, 13, dev), _song(m, 650, 3, 14, dev)]]
    try:
        det.force(True)
        m.use_graph = True
        captured, graphs = [], []
        for songs in calls:                               # both: B = 5, Lpad = 1024
            captured.append(m.sample_many([x[0] for x in songs], [x[1] for x in songs], 8, x_init=[x[2] for x in songs]))
            graphs.append(m._graph[1])
        assert graphs[0] is graphs[1]
        m.use_graph = False
        for songs, outs in zip(calls, captured):
            plain = m.sample_many([x[0] for x in songs], [x[1] for x in songs], 8, x_init=[x[2] for x in songs])
            for p, c in zip(plain, outs):
                assert torch.equal(p, c)
    finally:
        det.force(None)
        m.use_graph = True
