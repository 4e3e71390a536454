"""The latent model's forward kernels (osu_dreamer_amd/csrc/latent.hip: od_rmsnorm_affine_film, od_rmsnorm_affine_gate_residual, od_unet_mixer,
od_unet_down, od_unet_up, od_chart_head, od_attn_pool, od_spec_features_conv and their _varlen forms) against the formula in the header
comment of each kernel, evaluated in fp64 torch on the operands as the kernel reads them (rounded to bf16 in bf16 mode).

Bounds (the project's own, test_latent_bwd_kernels.FRAME):
  outputs of the activation type   2e-5 relative L2 per frame in fp32 (kernel_backend.TOL), 2^-8 in bf16 (one rounding to 8 significant bits)
  fp32 outputs in both modes       2e-5: the chart head's (B, N, L) rows per frame, the pool's vector per (b, head) — nothing is rounded to bf16
A frame is measured against the reference frame itself; against the sum of the terms' magnitudes where the output is a sum whose terms
cancel (gate and mixer: |x| + |the normed branch|; down and up: |bias| + sum |w| |x|; pool: sum p |v|).  The chart head's frames are
measured against the reference frame itself, with one allowance: an absolute error of one smallest normal fp32, 2^-126, for a sigmoid
of a logit under -87, which fp32 flushes to 0.
Frames past lens[b] of a VL form must be exactly 0, and an empty sequence pools to exactly 0.
No bound here was set from a measured fp32-reference error: every case stays within the bounds above on the emulator and on the MI355X.

Memory contract: every operand and output sits in a NaN buffer (Fenced: column offset 8, a leading dimension larger than C, NaN rows
below; Flat: 64 NaN either side), outputs are prefilled with NaN, the padding of a VL operand is NaN.  Afterwards nothing outside the
output was written and nothing inside is NaN; every kernel is launched twice and must give the same bits.

Shapes.  G = C / 8 lanes own a frame (8 channels a lane, lanes_ok: C a power of two in 8 .. 512) and a 256-thread block owns
fpb(C) = 256 / G frames of the flat B L index: C 8 / 32 / 128 / 512 -> 256 / 64 / 16 / 4 (C = 8: one lane group of one lane; C = 512:
one wave per frame).  Dense cases take B = 3 and L = ceil((fpb + 3) / 3): more than one block, a ragged last one, and a block that
straddles a batch border where the ssg row changes; and B = 2, L = fpb: two blocks filled exactly (2 fpb has no factor 3).
For down the blocks walk the B Lo output frames, for up the B Li s output frames; Lo (Li) is 1 (every tap an edge tap), 2, and a length
that crosses a block.  The strides run 1 .. 8 (the launchers' limit; ks = 1 + 2 (s / 2) taps).  The chart head takes N <= NMAX = 16.
The pool runs one block per (b, head), a thread per feature (hd <= 256) and chunks of 256 frames: L = 1, 255, 256, 257, 600.
SpecFeatures owns SF_TL = 64 frames of a batch row per block with a 2-frame halo, SF_F = 72 bins: L = 1, 2, 63, 64, 65, 130.
VL cases take B = 5 with lens = the padded length, 0, 1, and ends one frame either side of a block edge (of the flat index for the row
kernels, of the pool's chunk, of the SpecFeatures tile); the mixer's VL form maps five decoder rows onto three songs' skip rows.
test_latent_constants_match_sources re-reads these constants from latent.hip.

Frame families inside one input (frame i of the flat index): N(0, 1), amplitude 1e-3 (mean square ~ eps = 1e-6, so a missing or
misplaced eps shows at 2e-5), amplitude 1e3, and one all-zero frame (a finite result).  The chart head adds rows that drive one logit
to +-40 (the sigmoid saturates: exactly 1 above, no more than 2 exp(logit) below, never NaN).  Pool scores: 3 N(0, 1); the same +-100
(without the max subtraction exp overflows / the result is 0 / 0); one frame 50 above the rest in the last partial chunk; all equal
(the plain mean).  Spectrogram: runs of eight frames of amplitude 1, 1e-3, 1e2, and a run of all-zero frames (a bias-only output);
the biases are small (b1 1e-5, b2 1e-3), so that the 1e-3 frames bring the first norm's mean square to ~eps and the zero run the
second's within reach of it.
"""
import os
import re
from dataclasses import dataclass

import pytest
import torch
import torch.nn.functional as F_

from osu_dreamer_amd import _lib, ops
from osu_dreamer_amd._lib import OD_ACT_NONE, OD_ACT_SILU, HipKernelError
from osu_dreamer_amd.ops import _p, _stream
from kernel_backend import NAN, REPO, dev  # noqa: F401
from test_latent_bwd_kernels import FRAME, resample, rms, rn
from test_row_paths import EPS, EPS32, TORCH, Fenced, Flat, bits, check_frames

TS = ("fp32", "bf16")
CS = (8, 32, 128, 512)
POOL_CHUNK, SF_TL, SF_F, NMAX, SMAX = 256, 64, 72, 16, 8
TINY = 2.0 ** -126


def fpb(C):
    return 256 // (C // 8)


def cdiv(a, b):
    return -(-a // b)


def _gen(device, seed):
    return torch.Generator(device=device).manual_seed(seed)


def amps(M, device):
    """(M, 1) amplitudes: the frame families 1, 1e-3, 1e3 in turn and one all-zero frame."""
    a = torch.tensor([1.0, 1e-3, 1e3], device=device)[torch.arange(M, device=device) % 3]
    a[M // 2] = 0
    return a[:, None]


def edge_lens(B, L, f):
    """lens of B = 5 rows of L frames each, blocks of f frames of the flat index: L, 0, 1, and two ends one frame either side of the
    first block edge inside rows 3 and 4."""
    assert B == 5 and L >= f + 1
    e = [(b * L // f + 1) * f - b * L for b in (3, 4)]          # 1 <= e <= f
    return [L, 0, 1, e[0] - 1, e[1] + 1]


def valid_rows(lens, L, device):
    """(B L,) bool: frame l of row b is valid."""
    return (torch.arange(L, device=device)[None] < torch.tensor(lens, device=device)[:, None]).reshape(-1)


def i32(v, device):
    return torch.tensor(v, dtype=torch.int32, device=device)


def same_bits(case, a, b):
    assert torch.equal(bits(a.buf), bits(b.buf)), f"{case}: two launches differ"


def zero_padding(case, what, out, pad):
    n = int((out[pad] != 0).sum())
    assert n == 0, f"{case}: {n} elements of {what} past lens are not 0"


@dataclass(frozen=True)
class K:
    kind: str
    T: str
    B: int
    L: int
    C: int = 0
    vl: bool = False
    ssg: bool = True
    act: bool = False
    inplace: bool = False
    skip: str = "row"         # mixer: row / bcast / prow
    stride: int = 2
    N: int = 9
    nsig: int = 0
    rms: bool = False
    heads: int = 2
    hd: int = 8
    fam: str = "normal3"

    @property
    def id(self):
        ex = {"film": f"-ssg{int(self.ssg)}-silu{int(self.act)}", "gate": f"-ssg{int(self.ssg)}-{'in' if self.inplace else 'out'}place",
              "mixer": f"-{self.skip}-{'in' if self.inplace else 'out'}place", "down": f"-s{self.stride}", "up": f"-s{self.stride}",
              "head": f"-N{self.N}-sig{self.nsig}-rms{int(self.rms)}", "pool": f"-{self.fam}-{self.heads}x{self.hd}", "spec": ""}[self.kind]
        shape = f"{self.B}x{self.L}" + (f"x{self.C}" if self.C else "")         # spec and pool have no C
        return f"{self.kind}{'_vl' if self.vl else ''}-{self.T}{ex}-{shape}"


# ---------------------------------------------------------------- norm + FiLM (+ SiLU)
def run_film(c: K, device):
    B, L, C, tt, case = c.B, c.L, c.C, TORCH[c.T], c.id
    M = B * L
    g = _gen(device, 201)
    bi = torch.arange(M, device=device) // L
    lens = edge_lens(B, L, fpb(C)) if c.vl else [L] * B
    ok = valid_rows(lens, L, device)
    x0 = rn(g, device, M, C) * amps(M, device)
    x0[~ok] = NAN
    x = Fenced(M, C, tt, device, x0)
    gamma = Flat((C,), device, 1 + 0.2 * rn(g, device, C))
    ssg = Flat((B, 3 * C), device, rn(g, device, B, 3 * C, scale=0.5)) if c.ssg else None
    ref = rms(x.v.double()) * gamma.v.double()
    if c.ssg:
        sd = ssg.v.double()
        ref = ref * (1 + sd[bi, :C]) + sd[bi, C:2 * C]
    ref = F_.silu(ref) if c.act else ref
    ref[~ok] = 0
    act = OD_ACT_SILU if c.act else OD_ACT_NONE
    lt = i32(lens, device)

    def launch():
        y = Fenced(M, C, tt, device)
        if c.vl:
            ops.rmsnorm_affine_film_varlen(x.v, gamma.v, ssg.v if c.ssg else None, y.v, lt, B, L, act=act, eps=EPS)
        else:
            ops.rmsnorm_affine_film(x.v, gamma.v, ssg.v if c.ssg else None, y.v, B, L, act=act, eps=EPS)
        return y
    y = launch()
    y.check(case, "y")
    check_frames(case, "y", y.v, ref, FRAME[c.T])
    zero_padding(case, "y", y.v, ~ok)
    same_bits(case, y, launch())


# ---------------------------------------------------------------- norm + gate + residual
def run_gate(c: K, device):
    B, L, C, tt, case = c.B, c.L, c.C, TORCH[c.T], c.id
    M = B * L
    g = _gen(device, 202)
    bi = torch.arange(M, device=device) // L
    h = Fenced(M, C, tt, device, rn(g, device, M, C) * amps(M, device))
    x0 = rn(g, device, M, C).to(tt)
    gamma = Flat((C,), device, 1 + 0.2 * rn(g, device, C))
    ssg = Flat((B, 3 * C), device, rn(g, device, B, 3 * C, scale=0.5)) if c.ssg else None
    br = rms(h.v.double()) * gamma.v.double()
    if c.ssg:
        br = br * (1 + ssg.v.double()[bi, 2 * C:])
    ref, scale = x0.double() + br, x0.double().abs() + br.abs()

    def launch():
        x = Fenced(M, C, tt, device, x0)
        xo = x if c.inplace else Fenced(M, C, tt, device)
        ops.rmsnorm_affine_gate_residual(x.v, h.v, gamma.v, ssg.v if c.ssg else None, xo.v, B, L, eps=EPS)
        if not c.inplace:
            assert torch.equal(bits(x.v), bits(x0)), f"{case}: x was changed"
        return xo
    xo = launch()
    xo.check(case, "xo")
    check_frames(case, "xo", xo.v, ref, FRAME[c.T], scale)
    same_bits(case, xo, launch())


# ---------------------------------------------------------------- mixer
PROW = [0, 0, 1, 2, 2]


def run_mixer(c: K, device):
    B, L, C, tt, case = c.B, c.L, c.C, TORCH[c.T], c.id
    M = B * L
    g = _gen(device, 203)
    m = torch.arange(M, device=device)
    if c.skip == "prow":
        assert B == len(PROW)
        Mp, pr = 3 * L, torch.tensor(PROW, device=device)[m // L] * L + m % L
    elif c.skip == "bcast":
        Mp, pr = L, m % L
    else:
        Mp, pr = M, m
    p = Fenced(Mp, C, tt, device, rn(g, device, Mp, C) * amps(Mp, device))
    gx = Fenced(M, C, tt, device, rn(g, device, M, C))
    x0 = rn(g, device, M, C).to(tt)
    gamma = Flat((C,), device, 1 + 0.2 * rn(g, device, C))
    br = (rms(p.v.double()) * gamma.v.double())[pr] * gx.v.double()
    ref, scale = x0.double() + br, x0.double().abs() + br.abs()
    prow = i32(PROW, device)

    def launch():
        x = Fenced(M, C, tt, device, x0)
        xo = x if c.inplace else Fenced(M, C, tt, device)
        if c.skip == "prow":
            ops.unet_mixer_varlen(x.v, p.v, prow, gx.v, gamma.v, xo.v, B, L, eps=EPS)
        else:
            ops.unet_mixer(x.v, p.v, c.skip == "bcast", gx.v, gamma.v, xo.v, B, L, eps=EPS)
        return xo
    xo = launch()
    xo.check(case, "xo")
    check_frames(case, "xo", xo.v, ref, FRAME[c.T], scale)
    same_bits(case, xo, launch())


# ---------------------------------------------------------------- down / up
def resample64(x, w, b, s, up):
    """test_latent_bwd_kernels.resample — avg_pool1d(conv1d(x, padding=s // 2, groups=C), s), conv1d(interpolate(x, nearest), ...) —
    with the depthwise conv1d written as its sum over the taps, ks vectorised adds in place of a grouped conv1d of C groups.
    test_reference_conv_is_conv1d holds the two together."""
    r = s // 2
    x = F_.interpolate(x, scale_factor=s, mode="nearest") if up else x
    n, xp = x.shape[2], F_.pad(x, (r, r))
    y = b[None, :, None] + sum(w[None, :, 0, k, None] * xp[:, :, k:k + n] for k in range(2 * r + 1))
    return y if up else F_.avg_pool1d(y, s)


def test_reference_conv_is_conv1d():
    g = _gen("cpu", 208)
    for s in range(1, SMAX + 1):
        x, w, b = (torch.randn(*sh, generator=g, dtype=torch.float64) for sh in ((2, 16, 3 * s), (16, 1, 2 * (s // 2) + 1), (16,)))
        for up in (False, True):
            a, ref = resample64(x, w, b, s, up), resample(x, w, b, s, up)
            assert a.shape == ref.shape and float((a - ref).abs().max()) <= 1e-14 * float(ref.abs().max()), (s, up)


def run_resample(c: K, device):
    """c.L: the frames of the COARSE side per batch row (down: Lo, the output; up: Li, the input).  VL lens live at the input level."""
    up = c.kind == "up"
    B, Lc, C, s, tt, case = c.B, c.L, c.C, c.stride, TORCH[c.T], c.id
    ks, Lf = 2 * (s // 2) + 1, c.L * c.stride
    Lx, Ly = (Lc, Lf) if up else (Lf, Lc)
    g = _gen(device, 204)
    if c.vl:         # the outputs end either side of a block edge of the output frames; down: the input ends off a multiple of s
        e = edge_lens(B, Ly, fpb(C))
        lens = [Lc, 0, 1, e[3] // s, min(cdiv(e[4], s), Lc)] if up else [Lf, 0, 1, s * e[3] + (s > 1), min(s * e[4] + (s > 1), Lf)]
    else:
        lens = [Lx] * B
    x0 = rn(g, device, B * Lx, C) * amps(B * Lx, device)
    x0[~valid_rows(lens, Lx, device)] = NAN
    x = Fenced(B * Lx, C, tt, device, x0)
    w, bias = Flat((C, 1, ks), device, rn(g, device, C, 1, ks, scale=0.4)), Flat((C,), device, rn(g, device, C))     # distinct per channel
    xd = x.v.double().reshape(B, Lx, C).permute(0, 2, 1)
    ref, scale = (torch.zeros(B, Ly, C, dtype=torch.float64, device=device) for _ in range(2))
    nout = [n * s if up else n // s for n in lens]
    for b in range(B):       # each sequence alone
        if nout[b]:
            xb = xd[b:b + 1, :, :lens[b]]
            ref[b, :nout[b]] = resample64(xb, w.v.double(), bias.v.double(), s, up)[0].t()
            scale[b, :nout[b]] = resample64(xb.abs(), w.v.double().abs(), bias.v.double().abs(), s, up)[0].t()
    lt = i32(lens, device)

    def launch():
        y = Fenced(B * Ly, C, tt, device)
        if c.vl:
            (ops.unet_up_varlen if up else ops.unet_down_varlen)(x.v, w.v, bias.v, y.v, lt, B, Lc, s)
        else:
            (ops.unet_up if up else ops.unet_down)(x.v, w.v, bias.v, y.v, B, Lc, s)
        return y
    y = launch()
    y.check(case, "y")
    check_frames(case, "y", y.v, ref.reshape(B * Ly, C), FRAME[c.T], scale.reshape(B * Ly, C))
    zero_padding(case, "y", y.v, ~valid_rows(nout, Ly, device))
    same_bits(case, y, launch())


# ---------------------------------------------------------------- chart head (proj_out + sigmoid; temporal_head with its RMS norm)
def run_head(c: K, device):
    B, L, C, N, tt, case = c.B, c.L, c.C, c.N, TORCH[c.T], c.id
    M = B * L
    g = _gen(device, 205)
    lens = edge_lens(B, L, fpb(C)) if c.vl else [L] * B
    ok = valid_rows(lens, L, device)
    W = Flat((N, C), device, rn(g, device, N, C, scale=0.3))
    # with the norm the 1e-3 frames must reach a mean square of ~eps after the projection: the bias is as small as they are
    bias = Flat((N,), device, rn(g, device, N, scale=1e-3 if c.rms else 1.0))
    x0 = rn(g, device, M, C) * amps(M, device)
    sat = torch.arange(2, M, 4, device=device)          # rows that drive one logit (a sigmoid's, where there is one) to +40 and -40 in turn
    k = torch.arange(len(sat), device=device)
    wn = W.v[k % max(c.nsig, 1)]
    x0[sat] = (40.0 * (1 - 2 * (k % 2)).float())[:, None] * wn / wn.pow(2).sum(1, keepdim=True)
    x0[M // 2 + (M // 2 % 4 == 2)] = 0
    x0[~ok] = NAN
    x = Fenced(M, C, tt, device, x0)
    lg = x.v.double() @ W.v.double().t() + bias.v.double()
    sg = torch.sigmoid(lg[:, :c.nsig])
    y = torch.cat([sg, lg[:, c.nsig:]], 1)
    ref = y * torch.rsqrt(y.pow(2).mean(1, keepdim=True) + EPS32) if c.rms else y
    ref[~ok] = 0
    # the frame is measured against itself; the floor leaves one smallest normal fp32 of absolute error to a sigmoid of a logit under
    # -87, which fp32 flushes to 0
    scale = ref.abs().clamp_min(TINY / FRAME["fp32"])
    lt = i32(lens, device)

    def launch():
        out = Flat((B, N, L), device)
        if c.vl:
            ops.chart_head_varlen(x.v, W.v, bias.v, out.v, lt, B, L, c.nsig, rms=c.rms, eps=EPS)
        else:
            ops.chart_head(x.v, W.v, bias.v, out.v, B, L, c.nsig, rms=c.rms, eps=EPS)
        return out
    out = launch()
    out.check(case, "out")
    o = out.v.permute(0, 2, 1).reshape(M, N)
    check_frames(case, "out", o, ref, FRAME["fp32"], scale)
    zero_padding(case, "out", o, ~ok)
    if c.nsig and not c.rms:
        os_, ls = o[ok][:, :c.nsig], lg[ok][:, :c.nsig]
        assert bool((os_[ls >= 20] == 1).all()), f"{case}: a sigmoid above 20 is not exactly 1"
        low = ls <= -20
        assert bool(((os_[low] >= 0) & (os_[low].double() <= 2 * ls[low].exp())).all()), f"{case}: a sigmoid below -20 is not ~exp(logit)"
        assert int((ls >= 20).sum()) and int(low.sum()), f"{case}: no saturated logits"
    same_bits(case, out, launch())


# ---------------------------------------------------------------- AttnPool
def pool_scores(fam, B, L, Hh, g, device):
    s = rn(g, device, B, L, Hh, scale=3.0)
    if fam == "up100":
        s = s + 100
    elif fam == "dn100":
        s = s - 100
    elif fam == "spike":      # one frame 50 above the rest, in the last partial chunk of 256 (L = 256: the last chunk)
        s[:, L - 1 - (2 if (L - 1) % POOL_CHUNK >= 2 else 0)] = s.amax(1) + 50
    elif fam == "equal":
        s = torch.full_like(s, 0.75)
    return s.reshape(B * L, Hh)


def run_pool(c: K, device):
    B, L, Hh, hd, tt, case = c.B, c.L, c.heads, c.hd, TORCH[c.T], c.id
    M = B * L
    g = _gen(device, 206)
    lens = [L, 0, 1, POOL_CHUNK - 1, POOL_CHUNK + 1] if c.vl else [L] * B
    assert len(lens) == B and max(lens) <= L
    ok = valid_rows(lens, L, device)
    s0, v0 = pool_scores(c.fam, B, L, Hh, g, device), rn(g, device, M, Hh * hd)
    s0[~ok], v0[~ok] = NAN, NAN
    sc, va = Fenced(M, Hh, tt, device, s0), Fenced(M, Hh * hd, tt, device, v0)       # scores: a column view, lds > heads
    assert sc.v.stride(0) != Hh
    sd, vd = sc.v.double().reshape(B, L, Hh), va.v.double().reshape(B, L, Hh, hd)
    ref, scale = (torch.zeros(B, Hh, hd, dtype=torch.float64, device=device) for _ in range(2))
    for b in range(B):       # each sequence alone
        if lens[b]:
            p = torch.softmax(sd[b, :lens[b]], 0)
            ref[b] = torch.einsum("lh,lhd->hd", p, vd[b, :lens[b]])
            scale[b] = torch.einsum("lh,lhd->hd", p, vd[b, :lens[b]].abs())
    lt = i32(lens, device)

    def launch():
        out = Flat((B, Hh * hd), device)
        if c.vl:
            ops.attn_pool_varlen(sc.v, va.v, out.v, lt, B, L, Hh, hd)
        else:
            ops.attn_pool(sc.v, va.v, out.v, B, L, Hh, hd)
        return out
    out = launch()
    out.check(case, "out")
    check_frames(case, "out", out.v.reshape(B * Hh, hd), ref.reshape(B * Hh, hd), FRAME["fp32"], scale.reshape(B * Hh, hd))
    empty = torch.tensor([n == 0 for n in lens], device=device)
    zero_padding(case, "out", out.v, empty)
    same_bits(case, out, launch())


# ---------------------------------------------------------------- SpecFeatures: two strided Conv2d, each with a channel RMS norm and SiLU
def spec_ref(audio, P):
    """(B, 72, n) fp64 -> (B, n, 96): spec_features.py:17-26 as the oracle's spec_features writes it, 'b c a l -> b (c a) l', frame-major."""
    def cnorm(x, gm):        # RMS over the channels of (B, C, A, L)
        return x * torch.rsqrt(x.pow(2).mean(1, keepdim=True) + EPS32) * gm[None, :, None, None]
    h = F_.silu(cnorm(F_.conv2d(audio[:, None], P["w1"], P["b1"], stride=(6, 1), padding=(1, 1)), P["g1"]))
    h = F_.silu(cnorm(F_.conv2d(h, P["w2"], P["b2"], stride=(4, 1), padding=(1, 1)), P["g2"]))
    return h.flatten(1, 2).permute(0, 2, 1)


def run_spec(c: K, device):
    B, L, tt, case = c.B, c.L, TORCH[c.T], c.id
    M = B * L
    g = _gen(device, 207)
    lens = [L, 0, 1, SF_TL - 1, SF_TL + 1] if c.vl else [L] * B
    assert len(lens) == B and max(lens) <= L
    ok = valid_rows(lens, L, device)
    # runs of eight frames of amplitude 1, 1e-3, 1e2 along the flat frame index, and seven all-zero frames across the first tile border
    a = torch.tensor([1.0, 1e-3, 1e2], device=device)[torch.arange(M, device=device) // (8 if L >= 24 else 1) % 3]
    a = a.reshape(B, L).clone()
    z0 = max(min(SF_TL - 4, L - 7), 0)
    a[B - 1 if not c.vl else 0, z0:z0 + 7] = 0
    a0 = (rn(g, device, B, SF_F, L) * a[:, None]).masked_fill(~ok.reshape(B, 1, L), NAN)
    audio = Flat((B, SF_F, L), device, a0)
    shapes = {"w1": (8, 1, 8, 3), "b1": (8,), "g1": (8,), "w2": (32, 8, 6, 3), "b2": (32,), "g2": (32,)}
    # small biases: the 1e-3 frames bring the first norm's mean square to ~eps; in the zero run conv1 = b1 is far below sqrt(eps), the
    # first norm hands ~1e-2 on, and the second norm's mean square (b2 + w2 h1)^2 ~ 1e-4 is within reach of its eps
    amp = {"w1": 0.2, "w2": 0.2, "b1": 1e-5, "b2": 1e-3}
    P = {k: Flat(sh, device, (1 + 0.2 * rn(g, device, *sh)) if k[0] == "g" else rn(g, device, *sh, scale=amp[k])) for k, sh in shapes.items()}
    D = {k: v.v.double() for k, v in P.items()}
    ref = torch.zeros(B, L, 96, dtype=torch.float64, device=device)
    for b in range(B):       # each sequence alone
        if lens[b]:
            ref[b, :lens[b]] = spec_ref(audio.v.double()[b:b + 1, :, :lens[b]], D)[0]
    lt = i32(lens, device)

    def launch():
        out = Fenced(M, 96, tt, device)
        if c.vl:
            ops.spec_features_conv_varlen(audio.v, *(P[k].v for k in shapes), out.v, lt, eps=EPS)
        else:
            ops.spec_features_conv(audio.v, *(P[k].v for k in shapes), out.v, eps=EPS)
        return out
    out = launch()
    out.check(case, "out")
    check_frames(case, "out", out.v, ref.reshape(M, 96), FRAME[c.T])
    zero_padding(case, "out", out.v, ~ok)
    same_bits(case, out, launch())


RUN = {"film": run_film, "gate": run_gate, "mixer": run_mixer, "down": run_resample, "up": run_resample, "head": run_head,
       "pool": run_pool, "spec": run_spec}


# ---------------------------------------------------------------- the cases
def ragged(C):
    """L of a B = 3 batch of just over a block: B L > fpb, no multiple of it, and a block straddles a batch border."""
    return cdiv(fpb(C) + 3, 3)


def coarse_cross(kind, C, s):
    """The coarse length at which the B = 3 output frames of down / up cross a block without filling the last one."""
    per = 1 if kind == "down" else s
    n = cdiv(fpb(C) + 3, 3 * per)
    return n + (3 * n * per % fpb(C) == 0)


HEADS = ((9, 7, False), (6, 0, True), (16, 16, False))
HEADS_32 = ((1, 0, False), (1, 1, False), (1, 0, True), (16, 7, True), (9, 0, False), (6, 6, False), (9, 9, True), (16, 0, True), (16, 7, False))
POOLS = ((1, 1), (3, 20), (2, 256), (16, 64))
POOL_L = (1, 255, 256, 257, 600)
FAMS = ("normal3", "up100", "dn100", "spike", "equal")
SPEC_L = (1, 2, 63, 64, 65, 130)

CASES = []
for T in TS:
    for C in CS:
        f, r = fpb(C), ragged(C)
        CASES += [K("film", T, 3, r, C, ssg=a, act=b) for a in (True, False) for b in (True, False)]
        CASES += [K("film", T, 2, f, C, ssg=C in (8, 128), act=C in (8, 32))]
        CASES += [K("film", T, 5, f + 3, C, vl=True, ssg=C in (8, 128), act=C in (8, 128))]
        CASES += [K("gate", T, 3, r, C, ssg=a, inplace=a) for a in (True, False)] + [K("gate", T, 2, f, C, ssg=C in (8, 32), inplace=C in (8, 128))]
        CASES += [K("mixer", T, 3, r, C, skip="row", inplace=True), K("mixer", T, 3, r, C, skip="bcast", inplace=True),
                  K("mixer", T, 2, f, C, skip="bcast" if C in (32, 512) else "row", inplace=False),
                  K("mixer", T, 5, r, C, skip="prow", inplace=True)]
        CASES += [K("head", T, 3, r, C, N=n, nsig=q, rms=m) for n, q, m in HEADS[:2]] + [K("head", T, 2, f, C, N=16, nsig=16)]
        CASES += [K("head", T, 5, f + 3, C, vl=True, N=n, nsig=q, rms=m) for n, q, m in HEADS[C in (8, 128):][:1]]
    CASES += [K("head", T, 3, ragged(32), 32, N=n, nsig=q, rms=m) for n, q, m in HEADS_32]
    for kind in ("down", "up"):
        # every stride at C = 32 (fp32), 2 and 3 at the other widths, 3 and 4 in bf16; coarse lengths 1, 2 and across a block
        SC = [(s, 32) for s in range(1, SMAX + 1)] + [(s, C) for C in (8, 128, 512) for s in (2, 3)] if T == "fp32" else [(3, 32), (4, 32), (3, 128), (4, 8)]
        for s, C in SC:
            ns = {1, coarse_cross(kind, C, s)} | ({2} if s in (2, 3, 5, 8) else set()) if C == 32 else {coarse_cross(kind, C, s)} | ({1} if s == 2 else set())
            CASES += [K(kind, T, 3, n, C, stride=s) for n in sorted(ns)]
        VS = [(2, 32), (3, 32), (5, 32), (8, 32), (2, 8), (3, 128), (2, 512)] if T == "fp32" else [(3, 32), (4, 128)]
        CASES += [K(kind, T, 5, cdiv(fpb(C) + 3, 1 if kind == "down" else s) + (kind == "up"), C, vl=True, stride=s) for s, C in VS]
    for i, (hh, L) in enumerate((p, L) for p in POOLS for L in POOL_L):
        CASES += [K("pool", T, 3, L, heads=hh[0], hd=hh[1], fam=FAMS[(i + i // 5 + 2 * (T == "bf16")) % 5])]    # every L meets four families
    CASES += [K("pool", T, 5, 600, vl=True, heads=hh[0], hd=hh[1], fam=fam) for hh, fam in (((16, 64), "normal3"), ((3, 20), "up100"), ((2, 256), "spike"))]
    CASES += [K("spec", T, 3, L) for L in SPEC_L] + [K("spec", T, 5, 130, vl=True)]
CASES = list(dict.fromkeys(CASES))

IDS = [c.id for c in CASES]
assert len(set(IDS)) == len(IDS), "duplicate case ids"


def test_cases_cover_the_shapes():
    assert 250 <= len(CASES) <= 340, len(CASES)
    by = lambda kind, vl=False: [c for c in CASES if c.kind == kind and c.vl == vl]  # noqa: E731
    for kind in ("film", "gate", "mixer", "head"):
        for T in TS:
            for C in CS:
                cs = [c for c in by(kind) if c.T == T and c.C == C]
                n = [c.B * c.L for c in cs]
                assert any(c.B == 3 and m > fpb(C) and m % fpb(C) for c, m in zip(cs, n)), (kind, T, C)
                assert any(m == 2 * fpb(C) for m in n), (kind, T, C)
                assert kind == "gate" or any(c.T == T and c.C == C for c in by(kind, True) + [c for c in by(kind) if c.skip == "prow"]), (kind, T, C)
    assert {(c.ssg, c.act) for c in by("film")} == {(a, b) for a in (0, 1) for b in (0, 1)}
    assert {(c.ssg, c.inplace) for c in by("gate")} == {(a, b) for a in (0, 1) for b in (0, 1)}
    assert {(c.skip, c.inplace) for c in by("mixer")} >= {("row", True), ("bcast", True), ("prow", True), ("row", False), ("bcast", False)}
    hs = {(c.N, c.nsig, c.rms) for c in by("head")}
    assert {n for n, _, _ in hs} == {1, 6, 9, 16} and {(n, q) for n, q, _ in hs} >= {(1, 0), (1, 1), (6, 0), (6, 6), (9, 0), (9, 7), (9, 9), (16, 0), (16, 7), (16, 16)}
    assert {(n, m) for n, _, m in hs} >= {(n, m) for n in (1, 6, 9, 16) for m in (False, True)}
    for kind in ("down", "up"):
        cs = by(kind)
        assert {c.stride for c in cs if c.C == 32 and c.T == "fp32"} == set(range(1, SMAX + 1))
        assert all({c.stride for c in cs if c.C == C and c.T == "fp32"} >= {2, 3} for C in CS)
        assert {c.stride for c in cs if c.T == "bf16"} == {3, 4}
        fr = (lambda c: c.B * c.L) if kind == "down" else (lambda c: c.B * c.L * c.stride)
        for s in range(1, SMAX + 1):
            assert 1 in {c.L for c in cs if c.stride == s and c.C == 32}
            assert any(fr(c) > fpb(c.C) and fr(c) % fpb(c.C) for c in cs if c.stride == s), (kind, s)
        assert {c.L for c in cs if c.C == 32} >= {1, 2} and {c.C for c in by(kind, True)} == set(CS)
    ps = by("pool")
    assert {(c.heads, c.hd, c.L, c.T) for c in ps} == {(h, d, L, T) for h, d in POOLS for L in POOL_L for T in TS}
    assert all({c.fam for c in ps if c.T == T} == set(FAMS) for T in TS)
    assert all(any(c.fam == "spike" and c.L > POOL_CHUNK for c in ps if c.T == T) for T in TS)        # the spike in a chunk after the first
    assert {(c.L, c.T) for c in by("spec")} == {(L, T) for L in SPEC_L for T in TS} and len(by("spec", True)) == 2


def test_latent_constants_match_sources():
    """The constants the shape table of this file was derived from are the ones in latent.hip."""
    src = open(os.path.join(REPO, "osu_dreamer_amd", "csrc", "latent.hip")).read()
    fwd = src[:src.index("// Backward (training) kernels")]
    kernels = re.findall(r"__global__ __launch_bounds__\((\d+)\) void (\w+)\(", fwd)
    assert [k for _, k in kernels] == ["rms_affine_film_kernel", "rms_affine_gate_res_kernel", "mixer_kernel", "unet_down_kernel", "unet_up_kernel",
                                       "chart_head_kernel", "attn_pool_kernel", "spec_conv_kernel"]
    assert {int(n) for n, _ in kernels} == {256}
    assert len(re.findall(r"dim3\(256\)", fwd)) == 15 and not re.findall(r"dim3\((?!256\))\d+\)", fwd)       # eight dense launches, seven VL
    for s in ("const int G = C >> 3;                                                       \\\n"
              "    const long m = (long)blockIdx.x * (256 / G) + threadIdx.x / G;              \\\n"
              "    const int c = (threadIdx.x % G) * 8;",
              "const long m = (long)blockIdx.x * (256 / G) + threadIdx.x / G;\n    const int c = (threadIdx.x % G) * 8;\n    if (m >= M) return;",
              "inline bool lanes_ok(int C) { return C >= 8 && C <= 512 && (C & (C - 1)) == 0; }",
              "inline unsigned row_grid(long M, int C) { const int rpb = 256 / (C >> 3); return (unsigned)((M + rpb - 1) / rpb); }",
              f"constexpr int SF_TL = {SF_TL}, SF_F = {SF_F}, SF_C1 = 8, SF_A1 = 12, SF_C2 = 32, SF_A2 = 3;",
              "dim3 grid((L + SF_TL - 1) / SF_TL, B);",
              "if (F != SF_F) return OD_ERR_UNSUPPORTED;",
              f"chart_head_kernel<T_, {NMAX}>", f"chart_head_kernel<T_, {NMAX}, true>",
              f"if (N < 1 || N > {NMAX}) return OD_ERR_UNSUPPORTED;",
              f"if (stride < 1 || stride > {SMAX}) return OD_ERR_UNSUPPORTED;",
              "const int G = C >> 3, r = s / 2, ks = 2 * r + 1, L = Lo * s;", "const int G = C >> 3, r = s / 2, ks = 2 * r + 1, L = Li * s;",
              f"for (int l0 = 0; l0 < Lv; l0 += {POOL_CHUNK}) {{", f"const int n = Lv - l0 < {POOL_CHUNK} ? Lv - l0 : {POOL_CHUNK};",
              f"for (int l = t; l < Lv; l += {POOL_CHUNK})",
              f"if (hd < 1 || hd > {POOL_CHUNK} || Hh < 1 || L < 1) return OD_ERR_UNSUPPORTED;",
              "dim3(Hh, B), dim3(256)"):
        assert s in fwd, s
    assert fwd.count("if (m >= M) return;") == 2 and fwd.count("OD_ROW_OF_LANE();") == 4
    assert fwd.count(f"if (stride < 1 || stride > {SMAX}) return OD_ERR_UNSUPPORTED;") == 4
    assert [fpb(C) for C in CS] == [256, 64, 16, 4]


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_latent_path(dev, case):
    RUN[case.kind](case, dev)


# ---------------------------------------------------------------- refusals: the library's error, and nothing written
def _refused(case, outs, call):
    with pytest.raises(HipKernelError):
        call()
    if outs[0].is_cuda:
        torch.cuda.synchronize()
    for o in outs:
        assert bool(torch.isnan(o.float()).all()), f"{case}: a refused call wrote its output"


def _row_calls(device, tt, C, ld=None, B=2, L=3, stride=2, N=9, null=False, alloc=2):
    """{name: (outputs, call)} of every row kernel (dense and VL) at width C; ld: the leading dimension of every activation (a multiple
    of 8 by default); null: the VL forms get a null lens / prow; alloc: the stride the buffers are sized for."""
    ld = ld or (C + 15) // 8 * 8
    M = B * L * alloc

    def act(fill):
        return torch.full((M, ld), fill, dtype=tt, device=device)[:, :C]
    x, h, y = act(0.5), act(0.25), act(NAN)
    gamma, w, bias = (torch.ones(n, device=device) for n in (C, C * 9, C))
    n = max(N, 1)            # N = 0: the buffers still hold a row, so that "nothing written" has something to look at
    W, hb, out = torch.ones(n, C, device=device), torch.ones(n, device=device), torch.full((B, n, L), NAN, device=device)
    lens = None if null else torch.ones(B, dtype=torch.int32, device=device)
    dt, st, e, lib = ops.dt_code(tt), _stream(x), EPS, _lib.lib()
    return {
        "film": ([y], lambda: ops.rmsnorm_affine_film(x, gamma, None, y, B, L)),
        "gate": ([y], lambda: ops.rmsnorm_affine_gate_residual(x, h, gamma, None, y, B, L)),
        "mixer": ([y], lambda: ops.unet_mixer(x, h, False, h, gamma, y, B, L)),
        "down": ([y], lambda: ops.unet_down(x, w, bias, y, B, L, stride)),
        "up": ([y], lambda: ops.unet_up(x, w, bias, y, B, L, stride)),
        "head": ([out], lambda: lib.od_chart_head(dt, _p(x), ld, _p(W), _p(hb), _p(out), B, L, C, N, 0, 0, e, st)),
        "film_vl": ([y], lambda: lib.od_rmsnorm_affine_film_varlen(dt, _p(x), ld, _p(gamma), None, _p(y), ld, _p(lens), B, L, C, e, 0, st)),
        "mixer_vl": ([y], lambda: lib.od_unet_mixer_varlen(dt, _p(x), ld, _p(h), ld, _p(lens), _p(h), ld, _p(gamma), _p(y), ld, B, L, C, e, st)),
        "down_vl": ([y], lambda: lib.od_unet_down_varlen(dt, _p(x), ld, _p(w), _p(bias), _p(y), ld, _p(lens), B, L, C, stride, st)),
        "up_vl": ([y], lambda: lib.od_unet_up_varlen(dt, _p(x), ld, _p(w), _p(bias), _p(y), ld, _p(lens), B, L, C, stride, st)),
        "head_vl": ([out], lambda: lib.od_chart_head_varlen(dt, _p(x), ld, _p(W), _p(hb), _p(out), _p(lens), B, L, C, N, 0, 0, e, st)),
    }


def _pool_calls(device, tt, hd, B=2, L=3, Hh=2, null=False):
    n = max(hd, 1)
    sc, va = torch.zeros(B * L, Hh, dtype=tt, device=device), torch.ones(B * L, Hh * n, dtype=tt, device=device)
    out = torch.full((B, Hh * n), NAN, device=device)
    lens = None if null else torch.ones(B, dtype=torch.int32, device=device)
    dt, st, lib = ops.dt_code(tt), _stream(sc), _lib.lib()
    return {"pool": ([out], lambda: ops.attn_pool(sc, va, out, B, L, Hh, hd)),
            "pool_vl": ([out], lambda: lib.od_attn_pool_varlen(dt, _p(sc), Hh, _p(va), Hh * n, _p(out), _p(lens), B, L, Hh, hd, st))}


def _spec_calls(device, tt, F=SF_F, B=2, L=3, null=False):
    audio = torch.ones(B, F, L, device=device)
    P = [torch.ones(n, device=device) for n in (8 * 8 * 3, 8, 8, 32 * 8 * 6 * 3, 32, 32)]
    out = torch.full((B * L, 96), NAN, dtype=tt, device=device)
    lens = None if null else torch.ones(B, dtype=torch.int32, device=device)
    dt, st, lib = ops.dt_code(tt), _stream(audio), _lib.lib()
    return {"spec": ([out], lambda: ops.spec_features_conv(audio, *P, out)),
            "spec_vl": ([out], lambda: lib.od_spec_features_conv_varlen(dt, _p(audio), *(_p(t) for t in P), _p(out), 96, _p(lens), B, F, L, EPS, st))}


def _all(case, calls, only=None):
    for name, (outs, call) in calls.items():
        if only is None or name.split("_")[0] in only:
            _refused(f"{case} {name}", outs, call)


@pytest.mark.parametrize("C", (4, 24, 96, 1024))
def test_refuses_width(dev, C):
    _all(f"C={C}", _row_calls(dev, torch.float32, C))


def test_refuses_leading_dimension(dev):
    for tt in (torch.float32, torch.bfloat16):
        _all("ld=36", _row_calls(dev, tt, 32, ld=36))


@pytest.mark.parametrize("stride", (0, 9))
def test_refuses_stride(dev, stride):
    _all(f"stride={stride}", _row_calls(dev, torch.float32, 32, stride=stride, alloc=9), only=("down", "up"))


@pytest.mark.parametrize("N", (0, 17))
def test_refuses_head_outputs(dev, N):
    _all(f"N={N}", _row_calls(dev, torch.float32, 32, N=N), only=("head",))


@pytest.mark.parametrize("hd", (0, 257))
def test_refuses_pool_width(dev, hd):
    _all(f"hd={hd}", _pool_calls(dev, torch.float32, hd))


def test_refuses_fp16(dev):
    tt = torch.float16
    _all("fp16", {**_row_calls(dev, tt, 32), **_pool_calls(dev, tt, 8), **_spec_calls(dev, tt)})


def test_refuses_null_lens(dev):
    tt = torch.float32
    calls = {**_row_calls(dev, tt, 32, null=True), **_pool_calls(dev, tt, 8, null=True), **_spec_calls(dev, tt, null=True)}
    vl = {k: v for k, v in calls.items() if k.endswith("_vl")}
    assert len(vl) == 7
    _all("null lens", vl)


def test_refuses_spectrogram_bins(dev):
    for F in (71, 73):
        _all(f"F={F}", _spec_calls(dev, torch.float32, F=F))
