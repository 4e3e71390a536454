"""LDM.sample_many and `predict` with several `--spec` files: the whole inference pipeline for several songs, the denoiser sampler as one
batched call, against LDM.sample / a single-`--spec` run per song.
  * LDM.sample_many of two songs (the ldm_tiny golden song and the same song cut shorter) == LDM.sample per song within test_ldm.py's bound
    (1e-4 rel-L2), with pinned noise; through the `dev` fixture, so on the emulator and on the MI355X;
  * `predict` with two `--spec` files writes two npz files, each within 1e-5 rel-L2 of a single-`--spec` run of that song with the same
    `--seed` (fp32, the CLI default); with one `--spec` the file name, keys and shapes stay as before.
"""
import numpy as np
import pytest
import torch

from kernel_backend import dev, rel_l2  # noqa: F401
from osu_dreamer_amd.ldm import LDM, ldm_args_from_dict, pad_to_multiple
from test_ldm import hparams, load, make_ldm, weights

BOUND = 1e-4


def _latent_len(m, audio):
    return m.latent.audio_encoder(pad_to_multiple(audio.float(), m.latent.chunk_size)[None])[1].shape[-1]


def test_ldm_sample_many_matches_sample_per_song(dev):
    fx, ld, sd, dd = load("ldm_tiny")
    m = make_ldm(fx, ld, sd, dd, dev)
    n = int(fx["num_steps"])
    audio, labels = fx["audio"].to(dev), fx["labels"].to(dev)
    L = audio.shape[-1]
    short = audio[:, : (2 * L) // 3].contiguous()
    g = torch.Generator().manual_seed(3)
    lab2 = labels[:1].clone()
    s2 = torch.randn(1, fx["s_init"].shape[-1], generator=g).to(dev)
    x2 = torch.randn(1, dd.emb_dim, _latent_len(m, short), generator=g).to(dev)
    s1, x1 = fx["s_init"].to(dev), fx["x_init"].to(dev)
    outs = m.sample_many([audio, short], [labels, lab2], n, s_init=[s1, s2], x_init=[x1, x2])
    assert len(outs) == 2
    for (chart, out_labels), (a, lab, s, x) in zip(outs, ((audio, labels, s1, x1), (short, lab2, s2, x2))):
        ref_chart, ref_labels = m.sample(a, lab, n, s_init=s, x_init=x)
        assert chart.shape == ref_chart.shape and chart.shape[-1] == a.shape[-1]
        assert rel_l2(chart, ref_chart) < BOUND
        assert rel_l2(out_labels, ref_labels) < BOUND
    # the golden song inside the batch still meets the reference's own run
    assert rel_l2(outs[0][0], fx["chart"]) < BOUND


@pytest.mark.gpu
def test_predict_several_specs(tmp_path):
    from osu_dreamer_amd import fit
    fx, ld, sd, dd = load("ldm_tiny")
    hp, w = hparams(ld, sd, dd), weights(fx, ld, sd, dd)
    ref = LDM(ldm_args_from_dict(hp))
    ref.load_state_dict(w, strict=False)
    art = str(tmp_path / "inference.pt")
    torch.save({"hparams": hp, "state_dict": ref.state_dict()}, art)
    spec = fx["audio"].numpy()
    specs = {"a.spec": spec, "b.spec": np.ascontiguousarray(spec[:, : (2 * spec.shape[-1]) // 3])}
    for name, sp in specs.items():
        np.save(tmp_path / f"{name}.npy", sp)
    diffs = ["--diff", "5.5", "9", "8", "4", "6", "--diff", "3.2", "7", "6", "4", "5"]
    base = ["predict", "--model-path", art, "--sample-steps", "3", "--seed", "7", "--device", "cuda"] + diffs
    singles = {}
    for name in specs:
        out = str(tmp_path / f"single_{name}.npz")
        fit.main(base + ["--spec", str(tmp_path / f"{name}.npy"), "--out", out])
        singles[name] = np.load(out)
        assert set(singles[name].files) == {"pred_signals", "pred_labels"}
        assert singles[name]["pred_signals"].shape == (2, 9, specs[name].shape[-1])
    out_dir = tmp_path / "many"
    fit.main(base + ["--spec", str(tmp_path / "a.spec.npy"), "--spec", str(tmp_path / "b.spec.npy"), "--out", str(out_dir)])
    for name in specs:
        z = np.load(out_dir / f"{name}.npz")
        assert set(z.files) == {"pred_signals", "pred_labels"}
        for k in z.files:
            assert z[k].shape == singles[name][k].shape
            assert rel_l2(torch.from_numpy(z[k]), torch.from_numpy(singles[name][k])) <= 1e-5, (name, k)
