"""Varlen forms of the latent model's kernels and of LatentModel.audio_encoder / decode / encode_chart (`lengths=`): G sequences of
different lengths stacked zero-padded in one call, through the `dev` fixture (emulator and MI355X).
  * each VL kernel on NaN-poisoned padding: valid frames bit for bit the plain kernel on that sequence alone (and the torch/fp64 formula
    within fp32 rounding), padded frames exactly 0;
  * model level: the batched calls against per-song calls (fp32 1e-5 rel-L2, bf16 2e-2), padding exactly 0, a song's outputs
    bit-identical when its batch-mates' content changes but not their lengths, and the latent_tiny golden song inside a 3-song batch
    still meeting the reference's own outputs.
"""
import pytest
import torch
import torch.nn.functional as F

from oracle import latent_oracle as LO
from osu_dreamer_amd import ops
from kernel_backend import dev, frames, unframes, rel_l2  # noqa: F401
from test_latent import load, make_model

NAN = float("nan")


def _stack(seqs, Lpad, fill=NAN):
    """(C, L_b) tensors -> (B, C, Lpad) with `fill` past each sequence's end."""
    out = torch.full((len(seqs), seqs[0].shape[0], Lpad), fill)
    for b, s in enumerate(seqs):
        out[b, :, :s.shape[-1]] = s
    return out


def _lens(lens, dev):
    return torch.tensor(lens, dtype=torch.int32, device=dev)


def _check_rows(y, B, Lpad, lens, ref_of):
    """y frame-major [B*Lpad][C] (device): frames < lens[b] == ref_of(b) ([lens[b]][C], bit for bit), frames past it exactly 0."""
    y = y.float().cpu().view(B, Lpad, -1)
    for b in range(B):
        assert torch.equal(y[b, :lens[b]], ref_of(b).float().cpu()), b
        assert bool((y[b, lens[b]:] == 0).all()), b


# ---------------------------------------------------------------------------------- kernels
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_spec_features_conv_varlen(dev, dtype):
    g = torch.Generator().manual_seed(11)
    P = LO.init_latent_params(LO.LATENT_TINY, 5)
    p = "audio_encoder.0.net."
    w = [P[p + k].to(dev) for k in ("1.weight", "1.bias", "2.gamma", "4.weight", "4.bias", "5.gamma")]
    lens, Lpad = [5, 70, 200], 200                # shorter than a time tile, ragged, the padded length (tiles wholly past 5 and 70)
    seqs = [torch.randn(LO.A_DIM, n, generator=g) for n in lens]
    out = torch.full((len(lens) * Lpad, 96), NAN, dtype=dtype, device=dev)
    ops.spec_features_conv_varlen(_stack(seqs, Lpad).to(dev), *w, out, _lens(lens, dev))

    def ref(b):
        o = torch.zeros(lens[b], 96, dtype=dtype, device=dev)
        ops.spec_features_conv(seqs[b][None].to(dev), *w, o)
        return o
    _check_rows(out, len(lens), Lpad, lens, ref)
    if dtype == torch.float32:                    # the formula itself, on the shortest sequence
        x = seqs[0][None, None].double()
        P64 = {k: v.double() for k, v in P.items()}
        x = F.silu(LO.rms_norm(F.conv2d(x, P64[p + "1.weight"], P64[p + "1.bias"], stride=(6, 1), padding=(1, 1)), P64[p + "2.gamma"]))
        x = F.silu(LO.rms_norm(F.conv2d(x, P64[p + "4.weight"], P64[p + "4.bias"], stride=(4, 1), padding=(1, 1)), P64[p + "5.gamma"]))
        assert rel_l2(out.cpu().view(3, Lpad, 96)[0, :lens[0]], x.flatten(1, 2)[0].T) < 2e-5


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_row_kernels_varlen(dev, dtype):
    g = torch.Generator().manual_seed(12)
    C, Lpad, lens = 32, 45, [9, 27, 45]
    B = len(lens)
    x = torch.randn(B * Lpad, C, generator=g).to(dtype)
    for b in range(B):
        x[b * Lpad + lens[b]:(b + 1) * Lpad] = NAN
    gamma, ssg = 1 + 0.2 * torch.randn(C, generator=g), 0.3 * torch.randn(B, 3 * C, generator=g)
    y = torch.full_like(x, NAN).to(dev)
    ops.rmsnorm_affine_film_varlen(x.to(dev), gamma.to(dev), ssg.to(dev), y, _lens(lens, dev), B, Lpad, act=ops.OD_ACT_SILU)

    def ref(b):
        o = torch.zeros(lens[b], C, dtype=dtype, device=dev)
        ops.rmsnorm_affine_film(x[b * Lpad:b * Lpad + lens[b]].contiguous().to(dev), gamma.to(dev), ssg[b:b + 1].to(dev), o, 1,
                                lens[b], act=ops.OD_ACT_SILU)
        return o
    _check_rows(y, B, Lpad, lens, ref)
    # mixer: 5 decoder rows of 2 songs read their own song's skip row
    prow = [0, 0, 0, 1, 1]
    Bd, G = len(prow), 2
    xd, gx = (torch.randn(Bd * Lpad, C, generator=g).to(dtype) for _ in range(2))
    p = torch.randn(G * Lpad, C, generator=g).to(dtype)
    out = torch.full_like(xd, NAN).to(dev)
    ops.unet_mixer_varlen(xd.to(dev), p.to(dev), _lens(prow, dev), gx.to(dev), gamma.to(dev), out, Bd, Lpad)
    for sg, rows in ((0, slice(0, 3)), (1, slice(3, 5))):
        nb = rows.stop - rows.start
        r = torch.zeros(nb * Lpad, C, dtype=dtype, device=dev)
        fr = slice(rows.start * Lpad, rows.stop * Lpad)
        ops.unet_mixer(xd[fr].contiguous().to(dev), p[sg * Lpad:(sg + 1) * Lpad].contiguous().to(dev), True, gx[fr].contiguous().to(dev),
                       gamma.to(dev), r, nb, Lpad)
        assert torch.equal(out[fr].cpu(), r.cpu()), sg
        ref64 = xd[fr].double().view(nb, Lpad, C) + LO.rms_norm(p[sg * Lpad:(sg + 1) * Lpad].double().T[None], gamma.double()).transpose(1, 2) \
            * gx[fr].double().view(nb, Lpad, C)
        assert rel_l2(out[fr].cpu().view(nb, Lpad, C), ref64) < (2e-5 if dtype == torch.float32 else 2e-2)


@pytest.mark.parametrize("stride", [3, 2, 5])
def test_unet_down_up_varlen(dev, stride):
    g = torch.Generator().manual_seed(13)
    C, Lo_pad = 32, 11
    lo_lens = [1, 5, Lo_pad]                      # one output frame, odd, the padded length
    B = len(lo_lens)
    ks = 1 + 2 * (stride // 2)
    w, bias = torch.randn(C, 1, ks, generator=g) * 0.5, torch.randn(C, generator=g) * 0.1
    # down: lengths at the input level
    lens = [n * stride for n in lo_lens]
    seqs = [torch.randn(C, n, generator=g) for n in lens]
    x = frames(_stack(seqs, Lo_pad * stride)).to(dev)
    y = torch.full((B * Lo_pad, C), NAN, device=dev)
    ops.unet_down_varlen(x, w.to(dev), bias.to(dev), y, _lens(lens, dev), B, Lo_pad, stride)

    def ref_down(b):
        o = torch.zeros(lo_lens[b], C, device=dev)
        ops.unet_down(frames(seqs[b][None]).to(dev), w.to(dev), bias.to(dev), o, 1, lo_lens[b], stride)
        return o
    _check_rows(y, B, Lo_pad, lo_lens, ref_down)
    for b in range(B):
        r = F.avg_pool1d(F.conv1d(seqs[b][None].double(), w.double(), bias.double(), padding=stride // 2, groups=C), stride)[0].T
        assert rel_l2(y.cpu().view(B, Lo_pad, C)[b, :lo_lens[b]], r) < 2e-5
    # up: lengths at the input level (lo_lens), outputs stride x as long
    seqs = [torch.randn(C, n, generator=g) for n in lo_lens]
    y = torch.full((B * Lo_pad * stride, C), NAN, device=dev)
    ops.unet_up_varlen(frames(_stack(seqs, Lo_pad)).to(dev), w.to(dev), bias.to(dev), y, _lens(lo_lens, dev), B, Lo_pad, stride)

    def ref_up(b):
        o = torch.zeros(lens[b], C, device=dev)
        ops.unet_up(frames(seqs[b][None]).to(dev), w.to(dev), bias.to(dev), o, 1, lo_lens[b], stride)
        return o
    _check_rows(y, B, Lo_pad * stride, lens, ref_up)
    for b in range(B):
        r = F.conv1d(F.interpolate(seqs[b][None].double(), scale_factor=stride, mode="nearest"), w.double(), bias.double(),
                     padding=stride // 2, groups=C)[0].T
        assert rel_l2(y.cpu().view(B, -1, C)[b, :lens[b]], r) < 2e-5


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_attn_pool_chart_head_varlen(dev, dtype):
    g = torch.Generator().manual_seed(14)
    heads, hd, C, Lpad = 3, 20, 32, 300
    lens = [1, 77, 300]
    B = len(lens)
    sc = [torch.randn(heads, n, generator=g) * 3 for n in lens]
    va = [torch.randn(heads * hd, n, generator=g) for n in lens]
    out = torch.full((B, heads * hd), NAN, device=dev)
    scf, vaf = frames(_stack(sc, Lpad)).to(dtype).to(dev), frames(_stack(va, Lpad)).to(dtype).to(dev)
    ops.attn_pool_varlen(scf, vaf, out, _lens(lens, dev), B, Lpad, heads, hd)
    for b in range(B):
        r = torch.zeros(1, heads * hd, device=dev)
        ops.attn_pool(frames(sc[b][None]).to(dtype).to(dev), frames(va[b][None]).to(dtype).to(dev), r, 1, lens[b], heads, hd)
        assert torch.equal(out[b:b + 1].cpu(), r.cpu()), b
        s64, v64 = sc[b].to(dtype).double(), va[b].to(dtype).double()
        r64 = torch.einsum("hl,hdl->hd", s64.softmax(-1), v64.unflatten(0, (heads, hd))).flatten()
        assert rel_l2(out[b].cpu(), r64) < 2e-5
    # a sequence with no frame pools to 0, not to 0/0; the others are untouched
    out0 = torch.full((B, heads * hd), NAN, device=dev)
    ops.attn_pool_varlen(scf, vaf, out0, _lens([0] + lens[1:], dev), B, Lpad, heads, hd)
    assert bool((out0[0] == 0).all()) and torch.equal(out0[1:].cpu(), out[1:].cpu())
    # chart head, both modes (sigmoid rows then raw rows; RMS-normed rows)
    for N, n_sig, rms in ((9, 7, False), (6, 0, True)):
        lens = [9, 20, 29]
        xs = [torch.randn(C, n, generator=g) for n in lens]
        W, bias = torch.randn(N, C, generator=g) / 5, torch.randn(N, generator=g)
        o = torch.full((B, N, 29), NAN, device=dev)
        ops.chart_head_varlen(frames(_stack(xs, 29)).to(dtype).to(dev), W.to(dev), bias.to(dev), o, _lens(lens, dev), B, 29, n_sig, rms=rms)
        for b in range(B):
            r = torch.zeros(1, N, lens[b], device=dev)
            ops.chart_head(frames(xs[b][None]).to(dtype).to(dev), W.to(dev), bias.to(dev), r, 1, lens[b], n_sig, rms=rms)
            assert torch.equal(o[b:b + 1, :, :lens[b]].cpu(), r.cpu()), (b, rms)
            assert bool((o[b, :, lens[b]:] == 0).all()), (b, rms)


# ---------------------------------------------------------------------------------- model level
def _songs(d, nchunks, seed):
    g = torch.Generator().manual_seed(seed)
    return [torch.randn(LO.A_DIM, n * d.chunk_size, generator=g) for n in nchunks]


def _encode_batched(m, audios, dev, pad=NAN):
    c = m.chunk_size
    lens = [a.shape[-1] for a in audios]
    Lpad = max(lens) + 2 * c                       # a padded length no song has: every song has padding
    return m.audio_encoder(_stack(audios, Lpad, pad).to(dev), lengths=lens), lens


def _levels(m, lens):
    return [[n // m.stride ** i for n in lens] for i in range(m.n_downs + 1)]


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_audio_encoder_decode_varlen(dev, dtype):
    fx, d, P = load("latent_tiny")
    m = make_model(d, P, dev)
    m.compute_dtype = None if dtype == torch.float32 else dtype
    tol = 1e-5 if dtype == torch.float32 else 2e-2
    audios = _songs(d, [1, 3, 5], 21)
    (skips, h), lens = _encode_batched(m, audios, dev)
    lv = _levels(m, lens)
    per = [m.audio_encoder(a[None].to(dev)) for a in audios]
    for g, (psk, ph) in enumerate(per):
        for i, sk in enumerate(skips):
            assert rel_l2(sk[g, :, :lv[i][g]].float(), psk[i][0].float()) < tol, (g, i)
            assert bool((sk[g, :, lv[i][g]:] == 0).all()), (g, i)
        assert rel_l2(h[g, :, :lv[-1][g]].float(), ph[0].float()) < tol, g
        assert bool((h[g, :, lv[-1][g]:] == 0).all()), g
    # decode: 2 + 1 + 3 rows (several difficulties per song), z NaN past each song's latent length
    Bg = [2, 1, 3]
    offs = [0, 2, 3, 6]
    g_ = torch.Generator().manual_seed(22)
    zs = [torch.randn(n, d.emb_dim, lv[-1][g], generator=g_) for g, n in enumerate(Bg)]
    ss = [torch.randn(n, d.style_dim, generator=g_) for n in Bg]
    lz = h.shape[-1]
    z = torch.full((6, d.emb_dim, lz), NAN)
    for g in range(3):
        z[offs[g]:offs[g + 1], :, :lv[-1][g]] = zs[g]
    chart, labels = m.decode(z.to(dev), torch.cat(ss).to(dev), skips=skips, lengths=lens, offs=offs)
    assert tuple(chart.shape) == (6, LO.X_DIM, max(lens) + 2 * d.chunk_size)
    for g in range(3):
        pc, pl = m.decode(zs[g].to(dev), ss[g].to(dev), skips=per[g][0])
        rows = slice(offs[g], offs[g + 1])
        assert rel_l2(chart[rows, :, :lens[g]], pc) < tol, g
        assert bool((chart[rows, :, lens[g]:] == 0).all()), g
        assert rel_l2(labels[rows], pl) < tol, g
    # decode_logits and the audio= form take the same varlen arguments
    lg = m.decode_logits(z.to(dev), torch.cat(ss).to(dev), skips=skips, lengths=lens, offs=offs)
    assert rel_l2(lg[:, LO.N_HIT:], chart[:, LO.N_HIT:]) < 1e-6
    c2, _ = m.decode(z.to(dev), torch.cat(ss).to(dev), audio=_stack(audios, max(lens) + 2 * d.chunk_size).to(dev), lengths=lens, offs=offs)
    assert torch.equal(c2, chart)


def test_varlen_isolation(dev):
    """Song 1's outputs do not change by one bit when songs 0 and 2 change content but keep their lengths."""
    fx, d, P = load("latent_tiny")
    m = make_model(d, P, dev)
    a = _songs(d, [2, 4, 3], 31)
    b = _songs(d, [2, 4, 3], 32)
    b[1] = a[1]
    (ska, ha), lens = _encode_batched(m, a, dev)
    ska, ha = [s.clone() for s in ska], ha.clone()
    (skb, hb), _ = _encode_batched(m, b, dev, pad=0.0)
    assert torch.equal(ha[1], hb[1]) and all(torch.equal(x[1], y[1]) for x, y in zip(ska, skb))
    assert not torch.equal(ha[0], hb[0])
    g = torch.Generator().manual_seed(33)
    z = torch.randn(3, d.emb_dim, ha.shape[-1], generator=g)
    s = torch.randn(3, d.style_dim, generator=g)
    ca, la = m.decode(z.to(dev), s.to(dev), skips=ska, lengths=lens)
    z2, s2 = torch.randn_like(z), torch.randn_like(s)
    z2[1], s2[1] = z[1], s[1]
    cb, lb = m.decode(z2.to(dev), s2.to(dev), skips=skb, lengths=lens)
    assert torch.equal(ca[1], cb[1]) and torch.equal(la[1], lb[1])
    charts = [torch.rand(LO.X_DIM, n * d.chunk_size, generator=g) for n in (2, 4, 3)]
    charts2 = [torch.rand_like(c) for c in charts]
    charts2[1] = charts[1]
    Lpad = 6 * d.chunk_size
    za, sa = m.encode_chart(_stack(charts, Lpad).to(dev), lengths=lens)
    za, sa = za.clone(), sa.clone()
    zb, sb = m.encode_chart(_stack(charts2, Lpad, 0.0).to(dev), lengths=lens)
    assert torch.equal(za[1], zb[1]) and torch.equal(sa[1], sb[1])


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_encode_chart_varlen(dev, dtype):
    fx, d, P = load("latent_tiny")
    m = make_model(d, P, dev)
    m.compute_dtype = None if dtype == torch.float32 else dtype
    tol = 1e-5 if dtype == torch.float32 else 2e-2
    g = torch.Generator().manual_seed(41)
    lens = [d.chunk_size, 5 * d.chunk_size, 3 * d.chunk_size]
    charts = [torch.rand(LO.X_DIM, n, generator=g) for n in lens]
    z, s = m.encode_chart(_stack(charts, 6 * d.chunk_size).to(dev), lengths=lens)
    for b, c in enumerate(charts):
        pz, ps = m.encode_chart(c[None].to(dev))
        lz = lens[b] // d.chunk_size
        assert rel_l2(z[b:b + 1, :, :lz], pz) < tol and rel_l2(s[b:b + 1], ps) < tol, b
        assert bool((z[b, :, lz:] == 0).all()), b


def test_golden_song_inside_batch(dev):
    """latent_tiny (1 song, 3 difficulty rows) as the middle song of a 3-song batch meets the reference's own outputs."""
    fx, d, P = load("latent_tiny")
    m = make_model(d, P, dev)
    gold = fx["audio"][0]
    others = _songs(d, [2, 9], 51)
    audios = [others[0], gold, others[1]]
    (skips, h), lens = _encode_batched(m, audios, dev)
    lv = _levels(m, lens)
    for i, sk in enumerate(skips):
        assert rel_l2(sk[1:2, :, :lv[i][1]], fx[f"skip{i}"]) < 2e-5, i
    assert rel_l2(h[1:2, :, :lv[-1][1]], fx["h"]) < 2e-5
    g = torch.Generator().manual_seed(52)
    z = torch.zeros(5, d.emb_dim, h.shape[-1])
    s = torch.randn(5, d.style_dim, generator=g)
    z[0, :, :lv[-1][0]] = torch.randn(d.emb_dim, lv[-1][0], generator=g)
    z[1:4, :, :lv[-1][1]] = fx["z"]
    s[1:4] = fx["s"]
    z[4, :, :lv[-1][2]] = torch.randn(d.emb_dim, lv[-1][2], generator=g)
    chart, labels = m.decode(z.to(dev), s.to(dev), skips=skips, lengths=lens, offs=[0, 1, 4, 5])
    assert rel_l2(chart[1:4, :, :lens[1]], fx["chart"]) < 2e-5
    assert rel_l2(labels[1:4], fx["labels"]) < 1e-5
    ch = fx["chart_in"]
    L = ch.shape[-1]
    charts = [torch.rand(LO.X_DIM, 2 * d.chunk_size, generator=g), ch[0], ch[1], ch[2], torch.rand(LO.X_DIM, 10 * d.chunk_size, generator=g)]
    ez, es = m.encode_chart(_stack(charts, 10 * d.chunk_size).to(dev), lengths=[c.shape[-1] for c in charts])
    assert rel_l2(ez[1:4, :, :L // d.chunk_size], fx["enc_z"]) < 2e-5 and rel_l2(es[1:4], fx["enc_s"]) < 2e-5


def test_varlen_argument_errors(dev):
    fx, d, P = load("latent_tiny")
    m = make_model(d, P, dev)
    c = d.chunk_size
    audio = torch.zeros(2, LO.A_DIM, 4 * c, device=dev)
    with pytest.raises(ValueError):
        m.audio_encoder(audio, lengths=[c, c + 1])             # not a multiple of chunk_size
    with pytest.raises(ValueError):
        m.audio_encoder(audio, lengths=[c, 5 * c])             # longer than the padded length
    with pytest.raises(ValueError):
        m.audio_encoder(audio, lengths=[c])                    # one per row
    skips, _ = m.audio_encoder(audio, lengths=[c, 4 * c])
    z, s = torch.zeros(3, d.emb_dim, 4, device=dev), torch.zeros(3, d.style_dim, device=dev)
    with pytest.raises(ValueError):
        m.decode(z, s, skips=skips, lengths=[c, 4 * c], offs=[0, 2, 2])   # offs must end at B
    with pytest.raises(ValueError):
        m.decode(z, s, skips=skips, offs=[0, 1, 3])                      # offs without lengths
