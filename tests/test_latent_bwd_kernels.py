"""The latent model's backward kernels (osu_dreamer_amd/csrc/latent.hip: od_rmsnorm_affine_film_bwd, od_rmsnorm_affine_gate_residual_bwd,
od_unet_mixer_bwd, od_unet_down_bwd, od_unet_up_bwd, od_chart_head_bwd, od_attn_pool_bwd, od_spec_features_conv_bwd,
od_proj_in_bwd_input, od_add_rows) against fp64 torch autograd of the forward's formula, evaluated on the operands as the kernel reads them (rounded to bf16 in bf16 mode).

Bounds (the project's own):
  per-frame outputs, fp32       2e-5 relative L2 per frame (kernel_backend.TOL)
  per-frame outputs, bf16       2^-8 relative L2 per frame: one rounding to 8 significant bits (test_gemm_paths.py's per-tile bound)
  sums over frames / the batch  per element, 2e-5 of |old| + sum |terms| (test_row_paths.py's rule): fp32 in both modes
A frame is measured against the reference frame itself; against a stated scale only where the reference cancels to zero by construction
(an accumulated dx: |old| + |delta|; the pool's dscores: p (|dot| + sum p |dot|), zero at L = 1).  od_add_rows is exact in fp32 and
one rounding of the exact sum in bf16 (half an ulp of 8 significant bits: 2^-8 per element).  Outputs sit in NaN-fenced buffers, the
scratch rows too; sums are prefilled with known values and must come out as prefill + sum; every kernel is launched twice and must give the same bits.

Shapes: a block owns F(C) = 256 / (C / 8) * 4 frames (C 16 / 32 / 128: 512 / 256 / 64), per batch row for the kernels with a per-batch
output.  Each kernel runs with a ragged last block behind a full one (F + 3 frames) and with blocks filled exactly (F frames).
The SpecFeatures backward owns 32 frames of a batch row per block: 37 frames (ragged, the halo crosses the block border), 64 (exact), 1.
"""
from dataclasses import dataclass

import pytest
import torch
import torch.nn.functional as F_

from osu_dreamer_amd import ops
from osu_dreamer_amd._lib import OD_ACT_NONE, OD_ACT_SILU
from kernel_backend import TOL, dev  # noqa: F401
from test_row_paths import EPS, EPS32, TORCH, Fenced, Flat, bits, check_elems, check_frames

FRAME = {"fp32": TOL[torch.float32], "bf16": 2.0 ** -8}
SUM = 2e-5
TS = ("fp32", "bf16")


def blk(C):
    return 256 // (C // 8) * 4


def _gen(device, seed):
    return torch.Generator(device=device).manual_seed(seed)


def rn(g, device, *shape, scale=1.0):
    return scale * torch.randn(*shape, generator=g, device=device)


def rms(x, eps=EPS32):
    return x * torch.rsqrt(x.pow(2).mean(-1, keepdim=True) + eps)


def leaf(t):
    return t.detach().double().requires_grad_(True)


def scratch(n, device):
    return Flat((n,), device)


def check_scratch(case, ws):
    assert bool(torch.isnan(ws.buf[:64]).all() & torch.isnan(ws.buf[64 + ws.n:]).all()), f"{case}: written outside the scratch rows"


def same_bits(case, first, second):
    for a, b in zip(first, second):
        assert torch.equal(bits(a.buf), bits(b.buf)), f"{case}: two launches differ"


def per_batch(terms, B, L):
    """(B L, n) per-frame terms -> (B, n) sums."""
    return terms.reshape(B, L, -1).sum(1)


@dataclass(frozen=True)
class K:
    kind: str
    T: str
    B: int
    L: int
    C: int
    ssg: bool = True
    act: bool = False
    acc: bool = False
    bcast: bool = False
    stride: int = 2
    N: int = 9
    rms: bool = False
    heads: int = 2
    hd: int = 8
    E: int = 8

    @property
    def id(self):
        ex = {"film": f"-ssg{int(self.ssg)}-silu{int(self.act)}-acc{int(self.acc)}", "gate": f"-ssg{int(self.ssg)}",
              "mixer": f"-bcast{int(self.bcast)}", "down": f"-s{self.stride}", "up": f"-s{self.stride}",
              "head": f"-N{self.N}-rms{int(self.rms)}", "pool": f"-{self.heads}x{self.hd}", "proj": f"-E{self.E}", "spec": "", "add": ""}[self.kind]
        return f"{self.kind}-{self.T}{ex}-{self.B}x{self.L}x{self.C}"


# ---------------------------------------------------------------- norm + FiLM, norm + gate + residual
def run_film(c: K, device):
    B, L, C, tt, case = c.B, c.L, c.C, TORCH[c.T], c.id
    M = B * L
    g = _gen(device, 101)
    bi = torch.arange(M, device=device) // L
    x, dy = Fenced(M, C, tt, device, rn(g, device, M, C)), Fenced(M, C, tt, device, rn(g, device, M, C))
    gamma = Flat((C,), device, 1 + 0.2 * rn(g, device, C))
    ssg = Flat((B, 3 * C), device, rn(g, device, B, 3 * C, scale=0.5)) if c.ssg else None
    xd, gd = leaf(x.v), leaf(gamma.v)
    sd = leaf(ssg.v) if c.ssg else None
    xh = rms(xd)
    sc = 1 + sd[bi, :C] if c.ssg else torch.ones_like(xh)
    u = xh * gd * sc + (sd[bi, C:2 * C] if c.ssg else 0)
    u.retain_grad()
    y = F_.silu(u) if c.act else u
    (y * dy.v.double()).sum().backward()
    du, xh, sc = u.grad, xh.detach(), sc.detach()
    old = rn(g, device, M, C).to(tt) if c.acc else None
    g0, s0 = rn(g, device, C), rn(g, device, B, 3 * C)
    n = ops.latent_bwd_ws_floats("film", B, L, C)

    def launch():
        dx, dg, ds, ws = Fenced(M, C, tt, device, old), Flat((C,), device, g0), Flat((B, 3 * C), device, s0), scratch(n, device)
        ops.rmsnorm_affine_film_bwd(x.v, gamma.v, ssg.v if c.ssg else None, dy.v, dx.v, dg.v, ds.v if c.ssg else None, ws.v, B, L,
                                    act=OD_ACT_SILU if c.act else OD_ACT_NONE, accumulate_dx=c.acc, eps=EPS)
        check_scratch(case, ws)
        return dx, dg, ds
    dx, dg, ds = launch()
    dx.check(case, "dx")
    dg.check(case, "dgamma")
    ds.check(case, "dssg")
    if c.acc:
        check_frames(case, "dx", dx.v, old.double() + xd.grad, FRAME[c.T], old.double().abs() + xd.grad.abs())
    else:
        check_frames(case, "dx", dx.v, xd.grad, FRAME[c.T])
    check_elems(case, "dgamma", dg.v, g0.double() + gd.grad, g0.double().abs() + (du * sc * xh).abs().sum(0), SUM)
    if c.ssg:
        own = torch.cat([du * xh * gd.detach(), du], 1)
        ref = s0.double()[:, :2 * C] + sd.grad[:, :2 * C]
        check_elems(case, "dssg", ds.v[:, :2 * C], ref, s0.double()[:, :2 * C].abs() + per_batch(own.abs(), B, L), SUM)
        assert torch.equal(ds.v[:, 2 * C:], s0[:, 2 * C:]), f"{case}: the gate columns of dssg were changed"
    else:
        assert torch.equal(ds.v, s0), f"{case}: dssg was written without ssg"
    same_bits(case, (dx, dg, ds), launch())


def run_gate(c: K, device):
    B, L, C, tt, case = c.B, c.L, c.C, TORCH[c.T], c.id
    M = B * L
    g = _gen(device, 102)
    bi = torch.arange(M, device=device) // L
    h, dxo = Fenced(M, C, tt, device, rn(g, device, M, C)), Fenced(M, C, tt, device, rn(g, device, M, C))
    gamma = Flat((C,), device, 1 + 0.2 * rn(g, device, C))
    ssg = Flat((B, 3 * C), device, rn(g, device, B, 3 * C, scale=0.5)) if c.ssg else None
    hd_, gd = leaf(h.v), leaf(gamma.v)
    sd = leaf(ssg.v) if c.ssg else None
    hh = rms(hd_)
    gt = 1 + sd[bi, 2 * C:] if c.ssg else torch.ones_like(hh)
    ((hh * gd * gt) * dxo.v.double()).sum().backward()
    hh, gt, dd = hh.detach(), gt.detach(), dxo.v.double()
    g0, s0 = rn(g, device, C), rn(g, device, B, 3 * C)
    n = ops.latent_bwd_ws_floats("gate", B, L, C)

    def launch():
        dh, dg, ds, ws = Fenced(M, C, tt, device), Flat((C,), device, g0), Flat((B, 3 * C), device, s0), scratch(n, device)
        ops.rmsnorm_affine_gate_residual_bwd(h.v, gamma.v, ssg.v if c.ssg else None, dxo.v, dh.v, dg.v, ds.v if c.ssg else None, ws.v, B, L,
                                             eps=EPS)
        check_scratch(case, ws)
        return dh, dg, ds
    dh, dg, ds = launch()
    dh.check(case, "dh")
    dg.check(case, "dgamma")
    ds.check(case, "dssg")
    check_frames(case, "dh", dh.v, hd_.grad, FRAME[c.T])
    check_elems(case, "dgamma", dg.v, g0.double() + gd.grad, g0.double().abs() + (dd * gt * hh).abs().sum(0), SUM)
    if c.ssg:
        ref = s0.double()[:, 2 * C:] + sd.grad[:, 2 * C:]
        check_elems(case, "dssg", ds.v[:, 2 * C:], ref, s0.double()[:, 2 * C:].abs() + per_batch((dd * gd.detach() * hh).abs(), B, L), SUM)
        assert torch.equal(ds.v[:, :2 * C], s0[:, :2 * C]), f"{case}: the scale / shift columns of dssg were changed"
    else:
        assert torch.equal(ds.v, s0), f"{case}: dssg was written without ssg"
    same_bits(case, (dh, dg, ds), launch())


# ---------------------------------------------------------------- mixer
def run_mixer(c: K, device):
    B, L, C, tt, case = c.B, c.L, c.C, TORCH[c.T], c.id
    M = B * L
    g = _gen(device, 103)
    Mp = L if c.bcast else M
    p = Fenced(Mp, C, tt, device, rn(g, device, Mp, C))
    gx, dxo = Fenced(M, C, tt, device, rn(g, device, M, C)), Fenced(M, C, tt, device, rn(g, device, M, C))
    gamma = Flat((C,), device, 1 + 0.2 * rn(g, device, C))
    # the skip rows as every decoder row reads them: one leaf per (b, l), so the broadcast's terms stay apart
    pd = leaf(p.v.repeat(B, 1) if c.bcast else p.v)
    qd, gd, dd = leaf(gx.v), leaf(gamma.v), dxo.v.double()
    ph = rms(pd)
    ((ph * gd * qd) * dd).sum().backward()
    g0 = rn(g, device, C)
    n = ops.latent_bwd_ws_floats("mixer", B, L, C, int(c.bcast))

    def launch():
        dp = Fenced(Mp, C, torch.float32 if c.bcast else tt, device)
        dgx, dg, ws = Fenced(M, C, tt, device), Flat((C,), device, g0), scratch(n, device)
        ops.unet_mixer_bwd(p.v, c.bcast, gx.v, gamma.v, dxo.v, dp.v, dgx.v, dg.v, ws.v, B, L, eps=EPS)
        check_scratch(case, ws)
        return dp, dgx, dg
    dp, dgx, dg = launch()
    dp.check(case, "dp")
    dgx.check(case, "dgx")
    dg.check(case, "dgamma")
    check_frames(case, "dgx", dgx.v, qd.grad, FRAME[c.T])
    if c.bcast:      # a sum over the batch: fp32, per element against the sum of the batch rows' magnitudes
        per = pd.grad.reshape(B, L, C)
        check_elems(case, "dp", dp.v, per.sum(0), per.abs().sum(0), SUM)
    else:
        check_frames(case, "dp", dp.v, pd.grad, FRAME[c.T])
    check_elems(case, "dgamma", dg.v, g0.double() + gd.grad, g0.double().abs() + (dd * ph.detach() * qd.detach()).abs().sum(0), SUM)
    same_bits(case, (dp, dgx, dg), launch())


# ---------------------------------------------------------------- down / up
def resample(x, w, b, s, up):
    """(B, C, L) fp64 through unet.py's down (conv, AvgPool1d) or up (nearest Upsample, conv)."""
    C, r = x.shape[1], s // 2
    if up:
        return F_.conv1d(F_.interpolate(x, scale_factor=s, mode="nearest"), w, b, padding=r, groups=C)
    return F_.avg_pool1d(F_.conv1d(x, w, b, padding=r, groups=C), s)


def run_resample(c: K, device):
    """c.L: the frames of the COARSE side per batch row (down: Lo, the output; up: Li, the input)."""
    up = c.kind == "up"
    B, Lc, C, s, tt, case = c.B, c.L, c.C, c.stride, TORCH[c.T], c.id
    ks, Lf = 2 * (s // 2) + 1, c.L * c.stride
    Lx, Ly = (Lc, Lf) if up else (Lf, Lc)
    g = _gen(device, 104)
    x, dy = Fenced(B * Lx, C, tt, device, rn(g, device, B * Lx, C)), Fenced(B * Ly, C, tt, device, rn(g, device, B * Ly, C))
    w = Flat((C, 1, ks), device, rn(g, device, C, 1, ks, scale=0.4))

    def cm(t, Lt):      # frame-major rows -> (B, C, L) fp64
        return t.double().reshape(B, Lt, C).permute(0, 2, 1)

    def grads(xv, wv, dv):
        xl, wl, bl = leaf(xv), leaf(wv), torch.zeros(C, dtype=torch.float64, device=device, requires_grad=True)
        (resample(xl, wl, bl, s, up) * dv).sum().backward()
        return xl.grad.permute(0, 2, 1).reshape(B * Lx, C), wl.grad, bl.grad
    ref = grads(cm(x.v, Lx), w.v, cm(dy.v, Ly))
    mag = grads(cm(x.v, Lx).abs(), w.v.abs(), cm(dy.v, Ly).abs())      # every product positive: the sums of |terms|
    w0, b0 = rn(g, device, C, 1, ks), rn(g, device, C)
    n = ops.latent_bwd_ws_floats(c.kind, B, Ly, C, s)

    def launch():
        dx, dw, db, ws = Fenced(B * Lx, C, tt, device), Flat((C, 1, ks), device, w0), Flat((C,), device, b0), scratch(n, device)
        (ops.unet_up_bwd if up else ops.unet_down_bwd)(x.v, w.v, dy.v, dx.v, dw.v, db.v, ws.v, B, Lc, s)
        check_scratch(case, ws)
        return dx, dw, db
    dx, dw, db = launch()
    dx.check(case, "dx")
    dw.check(case, "dw")
    db.check(case, "db")
    check_frames(case, "dx", dx.v, ref[0], FRAME[c.T])
    check_elems(case, "dw", dw.v, w0.double() + ref[1], w0.double().abs() + mag[1], SUM)
    check_elems(case, "db", db.v, b0.double() + ref[2], b0.double().abs() + mag[2], SUM)
    same_bits(case, (dx, dw, db), launch())


# ---------------------------------------------------------------- chart head (proj_out; temporal_head with its RMS norm)
def run_head(c: K, device):
    B, L, C, N, tt, case = c.B, c.L, c.C, c.N, TORCH[c.T], c.id
    M = B * L
    g = _gen(device, 105)
    x = Fenced(M, C, tt, device, rn(g, device, M, C))
    W, bias = Flat((N, C), device, rn(g, device, N, C, scale=0.3)), Flat((N,), device, rn(g, device, N))
    dout = Flat((B, N, L), device, rn(g, device, B, N, L))
    xd, Wd, bd = leaf(x.v), leaf(W.v), leaf(bias.v)
    y = xd @ Wd.t() + bd
    y.retain_grad()
    out = rms(y) if c.rms else y
    (out * dout.v.double().permute(0, 2, 1).reshape(M, N)).sum().backward()
    dyv = y.grad
    W0, b0 = rn(g, device, N, C), rn(g, device, N)
    n = ops.latent_bwd_ws_floats("head", B, L, C, N)

    def launch():
        dx, dW, db, ws = Fenced(M, C, tt, device), Flat((N, C), device, W0), Flat((N,), device, b0), scratch(n, device)
        ops.chart_head_bwd(x.v, W.v, bias.v, dout.v, dx.v, dW.v, db.v, ws.v, B, L, rms=c.rms, eps=EPS)
        check_scratch(case, ws)
        return dx, dW, db
    dx, dW, db = launch()
    dx.check(case, "dx")
    dW.check(case, "dW")
    db.check(case, "db")
    check_frames(case, "dx", dx.v, xd.grad, FRAME[c.T])
    check_elems(case, "dW", dW.v, W0.double() + Wd.grad, W0.double().abs() + dyv.abs().t() @ xd.detach().abs(), SUM)
    check_elems(case, "db", db.v, b0.double() + bd.grad, b0.double().abs() + dyv.abs().sum(0), SUM)
    same_bits(case, (dx, dW, db), launch())


# ---------------------------------------------------------------- AttnPool
def run_pool(c: K, device):
    B, L, Hh, hd, tt, case = c.B, c.L, c.heads, c.hd, TORCH[c.T], c.id
    M = B * L
    g = _gen(device, 106)
    sc, va = Fenced(M, Hh, tt, device, rn(g, device, M, Hh, scale=2.0)), Fenced(M, Hh * hd, tt, device, rn(g, device, M, Hh * hd))
    dout = Flat((B, Hh * hd), device, rn(g, device, B, Hh * hd))
    sd, vd, dd = leaf(sc.v), leaf(va.v), dout.v.double().reshape(B, Hh, hd)
    p = torch.softmax(sd.reshape(B, L, Hh), 1)
    v4 = vd.reshape(B, L, Hh, hd)
    (torch.einsum("blh,blhd->bhd", p, v4) * dd).sum().backward()
    dot = torch.einsum("bhd,blhd->blh", dd, v4.detach())
    pdet = p.detach()
    scale = (pdet * (dot.abs() + (pdet * dot.abs()).sum(1, keepdim=True))).reshape(M, Hh)

    def launch():
        ds, dv = Fenced(M, Hh, tt, device), Fenced(M, Hh * hd, tt, device)
        ops.attn_pool_bwd(sc.v, va.v, dout.v, ds.v, dv.v, B, L, Hh, hd)
        return ds, dv
    ds, dv = launch()
    ds.check(case, "dscores")
    dv.check(case, "dvalues")
    check_frames(case, "dscores", ds.v, sd.grad, FRAME[c.T], scale)
    check_frames(case, "dvalues", dv.v, vd.grad, FRAME[c.T])
    same_bits(case, (ds, dv), launch())


# ---------------------------------------------------------------- SpecFeatures: two strided Conv2d, each with a channel RMS norm and SiLU
def run_spec(c: K, device):
    B, L, tt, case = c.B, c.L, TORCH[c.T], c.id
    M = B * L
    g = _gen(device, 108)
    audio = Flat((B, 72, L), device, rn(g, device, B, 72, L))
    shapes = {"w1": (8, 1, 8, 3), "b1": (8,), "g1": (8,), "w2": (32, 8, 6, 3), "b2": (32,), "g2": (32,)}
    P = {k: Flat(sh, device, (1 + 0.2 * rn(g, device, *sh)) if k[0] == "g" else rn(g, device, *sh, scale=0.2)) for k, sh in shapes.items()}
    dout = Fenced(M, 96, tt, device, rn(g, device, M, 96))
    D = {k: leaf(v.v) for k, v in P.items()}

    def cnorm(x):        # RMS over the channels of (B, C, A, L)
        return x * torch.rsqrt(x.pow(2).mean(1, keepdim=True) + EPS32)
    x0 = audio.v.double()[:, None]
    c1 = F_.conv2d(x0, D["w1"], D["b1"], stride=(6, 1), padding=(1, 1))
    n1 = cnorm(c1)
    u1 = n1 * D["g1"][None, :, None, None]
    h1 = F_.silu(u1)
    c2 = F_.conv2d(h1, D["w2"], D["b2"], stride=(4, 1), padding=(1, 1))
    n2 = cnorm(c2)
    u2 = n2 * D["g2"][None, :, None, None]
    for t in (c1, u1, c2, u2):
        t.retain_grad()
    out = F_.silu(u2).reshape(B, 96, L).permute(0, 2, 1).reshape(M, 96)          # 'b c a l -> b (c a) l', frame-major
    (out * dout.v.double()).sum().backward()
    mag = {"w1": torch.nn.grad.conv2d_weight(x0.abs(), shapes["w1"], c1.grad.abs(), stride=(6, 1), padding=(1, 1)),
           "b1": c1.grad.abs().sum((0, 2, 3)), "g1": (u1.grad * n1.detach()).abs().sum((0, 2, 3)),
           "w2": torch.nn.grad.conv2d_weight(h1.detach().abs(), shapes["w2"], c2.grad.abs(), stride=(4, 1), padding=(1, 1)),
           "b2": c2.grad.abs().sum((0, 2, 3)), "g2": (u2.grad * n2.detach()).abs().sum((0, 2, 3))}
    old = {k: rn(g, device, *sh) for k, sh in shapes.items()}
    n = ops.latent_bwd_ws_floats("spec", B, L, 0)

    def launch():
        G, ws = {k: Flat(sh, device, old[k]) for k, sh in shapes.items()}, scratch(n, device)
        ops.spec_features_conv_bwd(audio.v, *(P[k].v for k in shapes), dout.v, *(G[k].v for k in shapes), ws.v, eps=EPS)
        check_scratch(case, ws)
        return tuple(G[k] for k in shapes)
    first = launch()
    for k, t in zip(shapes, first):
        t.check(case, "d" + k)
        check_elems(case, "d" + k, t.v, old[k].double() + D[k].grad, old[k].double().abs() + mag[k], SUM)
    same_bits(case, first, launch())


# ---------------------------------------------------------------- proj_in towards its input
def run_proj(c: K, device):
    B, L, C, E, tt, case = c.B, c.L, c.C, c.E, TORCH[c.T], c.id
    M = B * L
    g = _gen(device, 107)
    dx = Fenced(M, C, tt, device, rn(g, device, M, C))
    W = Flat((C, E), device, rn(g, device, C, E, scale=0.3))

    def launch():
        dxt = Flat((B, E, L), device)
        ops.proj_in_bwd_input(dx.v, W.v, dxt.v)
        return (dxt,)
    (dxt,) = launch()
    dxt.check(case, "dxt")
    ref = dx.v.double() @ W.v.double()
    check_frames(case, "dxt", dxt.v.permute(0, 2, 1).reshape(M, E), ref, FRAME["fp32"])
    same_bits(case, (dxt,), launch())


# ---------------------------------------------------------------- y += x where two gradients of one activation meet
def run_add(c: K, device):
    B, L, C, tt, case = c.B, c.L, c.C, TORCH[c.T], c.id
    n = B * L * C
    g = _gen(device, 109)
    x = Flat((n,), device, rn(g, device, n), dtype=tt)
    old = rn(g, device, n).to(tt)

    def launch():
        y = Flat((n,), device, old, dtype=tt)
        ops.add_rows(x.v, y.v)
        return (y,)
    (y,) = launch()
    y.check(case, "y")
    ref = old.double() + x.v.double()
    if c.T == "fp32":
        assert torch.equal(y.v, old + x.v), f"{case}: y is not the fp32 sum"
    else:       # one rounding of the exact sum to bf16: at most half an ulp, 2^-8 of the result, per element
        assert bool(((y.v.double() - ref).abs() <= 2.0 ** -8 * ref.abs()).all()), f"{case}: y is further than one bf16 rounding from x + y"
    same_bits(case, (y,), launch())


RUN = {"film": run_film, "gate": run_gate, "mixer": run_mixer, "down": run_resample, "up": run_resample, "head": run_head,
       "pool": run_pool, "proj": run_proj, "spec": run_spec, "add": run_add}

CASES = []
for T in TS:
    for C in (16, 32, 128):
        f = blk(C)
        # blocks per batch row: a ragged block behind a full one (B = 3: three batch rows meet in dgamma, none in dssg), and exact blocks
        CASES += [K("film", T, 3, f + 3, C, ssg=True, act=True, acc=True), K("film", T, 2, f, C, ssg=False, act=False, acc=False),
                  K("gate", T, 3, f + 3, C, ssg=True), K("gate", T, 2, f, C, ssg=False),
                  K("mixer", T, 3, f + 3, C, bcast=False), K("mixer", T, 3, f + 3, C, bcast=True), K("mixer", T, 3, f, C, bcast=C == 128),
                  # flat blocks over B L frames: 2 (f / 2 + 3) = f + 6 frames (ragged), 2 (f / 2) = f (exact)
                  K("head", T, 2, f // 2 + 3, C, N=9, rms=False), K("head", T, 2, f // 2, C, N=6, rms=True),
                  K("proj", T, 2, 37, C, E=8), K("proj", T, 1, 256 // (C // 8), C, E=6)]
    # the remaining combinations of ssg / act / accumulate, and of N / rms
    CASES += [K("film", T, 2, 37, 32, ssg=True, act=False, acc=False), K("film", T, 2, 37, 32, ssg=False, act=True, acc=True),
              K("film", T, 2, 37, 32, ssg=True, act=True, acc=False), K("film", T, 2, 37, 32, ssg=False, act=False, acc=True),
              K("film", T, 2, 37, 32, ssg=True, act=False, acc=True), K("film", T, 2, 37, 32, ssg=False, act=True, acc=False),
              K("head", T, 2, 37, 32, N=9, rms=True), K("head", T, 2, 37, 32, N=6, rms=False)]
    for kind in ("down", "up"):
        for s, C in ((2, 16), (3, 128), (4, 32), (2, 128), (3, 32), (4, 16)):
            f = blk(C)
            # c.L is the coarse length; the weight sums walk the frames of dy (down: B Lo, up: B Li s)
            per = f if kind == "down" else -(-f // s)
            CASES += [K(kind, T, 2, per // 2 + 3, C, stride=s)]
        # one coarse frame: the conv sees its own zero padding on both sides (down: L = stride in, 1 out; up: L = 1 in, stride out)
        CASES += [K(kind, T, 1, 1, 32, stride=s) for s in (2, 3, 4)] + [K(kind, T, 3, 1, 16, stride=3)]
    CASES += [K("down", T, 2, blk(128) // 2, 128, stride=3), K("up", T, 2, blk(32) // 8, 32, stride=4)]      # blocks filled exactly
    # C = 8, the narrowest width the head takes: one lane owns a frame and all 256 slots of a block hand db over
    CASES += [K("head", T, 2, blk(8) // 2 + 3, 8, N=9, rms=True), K("head", T, 1, blk(8), 8, N=16, rms=False)]
    # 8 elements (one thread), a ragged last block behind a full one (2048 elements a block), blocks filled exactly
    CASES += [K("add", T, 1, 1, 8), K("add", T, 3, 37, 32), K("add", T, 2, 64, 128)]
    CASES += [K("spec", T, 2, 37, 0), K("spec", T, 1, 64, 0), K("spec", T, 1, 1, 0)]
    for L in (1, 7, 300):
        CASES += [K("pool", T, 3, L, 0, heads=2, hd=8), K("pool", T, 3, L, 0, heads=16, hd=64)]

IDS = [c.id for c in CASES]
assert len(set(IDS)) == len(IDS), "duplicate case ids"


def test_cases_cover_the_shapes():
    for kind in ("film", "gate", "mixer", "head"):
        cs = [c for c in CASES if c.kind == kind]
        assert {c.C for c in cs} - {8} == {16, 32, 128}
        n = (lambda c: c.L) if kind != "head" else (lambda c: c.B * c.L)
        assert any(n(c) % blk(c.C) == 0 for c in cs) and any(n(c) > blk(c.C) and n(c) % blk(c.C) for c in cs), kind
    assert {(c.ssg, c.act, c.acc) for c in CASES if c.kind == "film"} == {(a, b, d) for a in (0, 1) for b in (0, 1) for d in (0, 1)}
    assert {(c.bcast, c.B) for c in CASES if c.kind == "mixer"} == {(False, 3), (True, 3)}
    assert {(c.N, c.rms) for c in CASES if c.kind == "head"} >= {(9, False), (9, True), (6, False), (6, True)}
    for kind in ("down", "up"):
        cs = [c for c in CASES if c.kind == kind]
        assert {c.stride for c in cs} == {2, 3, 4} and {c.stride for c in cs if c.L == 1} == {2, 3, 4}
        fr = (lambda c: c.B * c.L) if kind == "down" else (lambda c: c.B * c.L * c.stride)
        assert any(fr(c) % blk(c.C) == 0 for c in cs) and any(fr(c) > blk(c.C) and fr(c) % blk(c.C) for c in cs), kind
    assert {(c.heads, c.hd, c.L) for c in CASES if c.kind == "pool"} >= {(h, d, L) for h, d in ((2, 8), (16, 64)) for L in (1, 7)}


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_latent_bwd_kernel(dev, case):
    assert ops.latent_bwd_ws_floats("film", 1, 1, 128) == 3 * 128 and blk(128) == 64
    RUN[case.kind](case, dev)


def test_scratch_too_small_is_refused(dev):
    """A workspace shorter than the partial rows is an argument error, not a write past its end."""
    from osu_dreamer_amd._lib import HipKernelError
    C, B, L = 32, 2, 300
    t = lambda *s: torch.zeros(*s, device=dev)  # noqa: E731
    n = ops.latent_bwd_ws_floats("gate", B, L, C)
    with pytest.raises(HipKernelError):
        ops.rmsnorm_affine_gate_residual_bwd(t(B * L, C), t(C), None, t(B * L, C), t(B * L, C), t(C), None, t(n - 1), B, L)
