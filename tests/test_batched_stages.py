"""The stages of LDM.sample_many besides the denoiser, batched over songs: StyleModel.sample_many against StyleModel.sample per song,
and LDM.sample_many matching LDM.sample per song (test_ldm.py's 1e-4 rel-L2 in fp32) while entering the audio encoder and the style
sampler exactly once for all songs; the decoder once for all songs in bf16, once per song in fp32 (where a loop of per-song decoder
calls beats one padded call, profiles/r08_ldm_many.txt).  Through the `dev` fixture: emulator and MI355X."""
import os

import numpy as np
import torch

from oracle import style_oracle as SO
from osu_dreamer_amd.style import StyleModel, StyleModelArgs
from kernel_backend import dev, rel_l2  # noqa: F401
from test_ldm import load, make_ldm

GOLDEN = os.path.join(os.path.dirname(__file__), "golden")
BOUND = 1e-4


def _style_model(dev):
    z = np.load(os.path.join(GOLDEN, "style_tiny.npz"))
    fx = {k: torch.from_numpy(np.asarray(z[k])) for k in z.files}
    v_ = [int(x) for x in fx["dims"].tolist()]
    d = SO.StyleDims(style_dim=v_[0], label_features=v_[1], h_dim=v_[2], depth=v_[3], expand=v_[4])
    P = ({k[2:]: t for k, t in fx.items() if k.startswith("w.")} if any(k.startswith("w.") for k in fx)
         else SO.init_style_params(d, int(fx["seed"])))
    m = StyleModel(d.style_dim, StyleModelArgs(d.label_features, d.h_dim, d.depth, d.expand))
    m.load_state_dict(P)
    return m.to(dev), fx


def test_style_sample_many_matches_sample(dev):
    m, fx = _style_model(dev)
    g = torch.Generator().manual_seed(5)
    Bs = [3, 1, 4]
    labels = [torch.rand(n, 5, generator=g) * 10 for n in Bs]
    s_init = [torch.randn(n, m.style_dim, generator=g) for n in Bs]
    for steps in (16, 5):
        outs = m.sample_many([lab.to(dev) for lab in labels], steps, s_init=[s.to(dev) for s in s_init])
        assert [tuple(o.shape) for o in outs] == [(n, m.style_dim) for n in Bs]
        for lab, si, o in zip(labels, s_init, outs):
            ref = m.sample(lab.to(dev), steps, s_init=si.to(dev))
            assert rel_l2(o, ref) <= 1e-6
    # the golden song still meets the reference's own run from inside a batch
    outs = m.sample_many([labels[0].to(dev), fx["labels"].to(dev)], 16, s_init=[s_init[0].to(dev), fx["s_init"].to(dev)])
    assert rel_l2(outs[1], fx["sample_s"]) < 1e-4
    # without s_init: the noise G sample() calls would draw, in song order
    torch.manual_seed(9)
    drawn = m.sample_many([lab.to(dev) for lab in labels], 4)
    torch.manual_seed(9)
    pinned = [torch.randn(n, m.style_dim, device=dev) for n in Bs]
    again = m.sample_many([lab.to(dev) for lab in labels], 4, s_init=pinned)
    assert all(torch.equal(a, b) for a, b in zip(drawn, again))


def _count(obj, name, counts):
    fn = getattr(obj, name)

    def wrapped(*a, **k):
        counts[name] = counts.get(name, 0) + 1
        return fn(*a, **k)
    setattr(obj, name, wrapped)


def test_ldm_sample_many_batches_every_stage(dev):
    fx, ld, sd, dd = load("ldm_tiny")
    m = make_ldm(fx, ld, sd, dd, dev)
    n = int(fx["num_steps"])
    audio, labels = fx["audio"].to(dev), fx["labels"].to(dev)
    L = audio.shape[-1]
    g = torch.Generator().manual_seed(4)
    songs = [audio, audio[:, : L // 2].contiguous(), torch.rand(audio.shape[0], L + 13, generator=g).to(dev)]
    labs = [labels, labels[:1].clone(), (torch.rand(4, 5, generator=g) * 10).to(dev)]
    c = m.latent.chunk_size
    s_init = [fx["s_init"].to(dev)] + [torch.randn(lab.shape[0], sd.style_dim, generator=g).to(dev) for lab in labs[1:]]
    x_init = [fx["x_init"].to(dev)] + [torch.randn(lab.shape[0], dd.emb_dim, -(-a.shape[-1] // c), generator=g).to(dev)
                                       for a, lab in zip(songs[1:], labs[1:])]
    counts = {}
    _count(m.latent, "_audio_encoder", counts)
    _count(m.latent, "_decode", counts)
    _count(m.style, "sample", counts)
    _count(m.style, "sample_many", counts)
    outs = m.sample_many(songs, labs, n, s_init=s_init, x_init=x_init)
    assert counts.get("_audio_encoder") == 1 and counts.get("_decode") == len(songs), counts      # fp32: per-song decoder
    assert counts.get("sample", 0) + counts.get("sample_many", 0) == 1, counts
    assert len(outs) == 3
    for (chart, out_labels), a, lab, s, x in zip(outs, songs, labs, s_init, x_init):
        ref_chart, ref_labels = m.sample(a, lab, n, s_init=s, x_init=x)
        assert chart.shape == ref_chart.shape and chart.shape[-1] == a.shape[-1]
        assert rel_l2(chart, ref_chart) < BOUND
        assert rel_l2(out_labels, ref_labels) < BOUND
    assert rel_l2(outs[0][0], fx["chart"]) < BOUND
    # without pinned noise: the draws of G sample() calls (style noise per song, then latent noise per song)
    torch.manual_seed(11)
    drawn = m.sample_many(songs, labs, 2)
    torch.manual_seed(11)
    s2 = [torch.randn(lab.shape[0], sd.style_dim, device=dev) for lab in labs]
    x2 = [torch.randn(lab.shape[0], dd.emb_dim, -(-a.shape[-1] // c), device=dev) for a, lab in zip(songs, labs)]
    again = m.sample_many(songs, labs, 2, s_init=s2, x_init=x2)
    for (c1, l1), (c2, l2) in zip(drawn, again):
        assert torch.equal(c1, c2) and torch.equal(l1, l2)


def test_ldm_sample_many_bf16_decodes_once(dev):
    fx, ld, sd, dd = load("ldm_tiny")
    m = make_ldm(fx, ld, sd, dd, dev)
    m.set_precision(torch.bfloat16)
    audio, labels = fx["audio"].to(dev), fx["labels"].to(dev)
    L = audio.shape[-1]
    g = torch.Generator().manual_seed(6)
    songs = [audio, audio[:, : L // 2].contiguous(), torch.rand(audio.shape[0], L + 13, generator=g).to(dev)]
    labs = [labels, labels[:1].clone(), (torch.rand(4, 5, generator=g) * 10).to(dev)]
    c = m.latent.chunk_size
    s_init = [torch.randn(lab.shape[0], sd.style_dim, generator=g).to(dev) for lab in labs]
    x_init = [torch.randn(lab.shape[0], dd.emb_dim, -(-a.shape[-1] // c), generator=g).to(dev) for a, lab in zip(songs, labs)]
    counts = {}
    for obj, name in ((m.latent, "_audio_encoder"), (m.latent, "_decode"), (m.style, "sample"), (m.style, "sample_many")):
        _count(obj, name, counts)
    outs = m.sample_many(songs, labs, 2, s_init=s_init, x_init=x_init)
    assert counts.get("_audio_encoder") == 1 and counts.get("_decode") == 1, counts
    assert counts.get("sample", 0) + counts.get("sample_many", 0) == 1, counts
    for (chart, out_labels), a, lab, s, x in zip(outs, songs, labs, s_init, x_init):
        ref_chart, ref_labels = m.sample(a, lab, 2, s_init=s, x_init=x)
        assert chart.shape == ref_chart.shape
        assert rel_l2(chart, ref_chart) < 5e-2 and rel_l2(out_labels, ref_labels) < 5e-2
