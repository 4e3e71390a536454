"""The training-step kernels of LatentTrainer (osu_dreamer_amd/csrc/latent.hip: od_latent_perturb(+_bwd), od_latent_loss(+_bwd), od_mmd_imq,
od_scale_by) against fp64 restatements of the formulae, written here (latent/train.py:86-149 and common/wae.py:4-28 of the reference; the
reference itself is never imported).

Bounds:
  perturbation   the zeroed frames and the replaced rows equal the fp32 torch expression exactly; outputs within 1 ulp; backward exact
  loss           every component within 2e-5 of fp64 relative to sum |terms| / N (hit channels: sum |bce| + sum |floor|, the floor
                 subtraction cancels); all rows masked: label loss and gradient exactly 0; dlogits / dlabels 1e-5 relative L2 per channel;
                 the cursor stencil per frame at both ends of a row and on both sides of every tile boundary, 1e-5 of the row's rms (a frame's
                 gradient is a sum of at most 13 products of about that size, each rounded to 2^-24; a missing stencil term is of the order
                 of the rms itself)
  loss_ema, loss a handful of fp32 operations on the components the kernel reported: 1e-6 relative
  MMD            value within 2e-5 (|zz| + |pp| + 2 |zp|) of fp64; gradient 1e-3 relative L2
Every output sits in a fenced buffer (NaN, or a sentinel for integers), and every kernel is launched twice and must give the same bits.
"""
import math

import pytest
import torch
import torch.nn.functional as F

from osu_dreamer_amd import ops
from kernel_backend import dev, rel_l2  # noqa: F401

PAD = 64
SCALES = (.1, .2, .5, 1., 2., 5., 10.)
WEIGHTS = (1., 1., 1., 1., 1., 1., 1., 2., 2., 2., 2.)
ONE_MINUS = 1.0 - 2.0 ** -24            # the largest fp32 below 1


class Fenced:
    """A contiguous tensor inside a buffer whose margins hold a sentinel."""

    def __init__(self, shape, device, dtype=torch.float32):
        self.n = math.prod(shape)
        self.sent = float("nan") if dtype.is_floating_point else 0x5A
        self.buf = torch.full((self.n + 2 * PAD,), self.sent, dtype=dtype, device=device)
        self.t = self.buf[PAD:PAD + self.n].view(shape)

    def check(self, what):
        m = torch.cat([self.buf[:PAD], self.buf[PAD + self.n:]])
        ok = torch.isnan(m).all() if self.buf.dtype.is_floating_point else (m == self.sent).all()
        assert bool(ok), f"{what}: written outside the buffer"
        if self.buf.dtype.is_floating_point:
            assert not bool(torch.isnan(self.t).any()), f"{what}: an element was left unwritten (or is NaN)"


def bits(t):
    return t.contiguous().view(torch.int32) if t.dtype == torch.float32 else t


def gen(seed):
    return torch.Generator().manual_seed(seed)


def within_one_ulp(a, b):
    a, b = a.cpu(), b.cpu()
    lo, hi = torch.nextafter(b, torch.full_like(b, -math.inf)), torch.nextafter(b, torch.full_like(b, math.inf))
    return bool(((a >= lo) & (a <= hi)).all())


# ================================================================================================================ perturbation
def perturb_ref(z, s, eps_z, eps_s, u_s, repl, u_span, u_start, s_noise, z_noise, s_frac, z_frac, training):
    """latent/train.py:90-112 in fp32 torch on the CPU, draws pinned."""
    B2, _, l = z.shape
    s = s.view(B2 // 2, 2, -1).flip(1).reshape(B2, -1)
    masked = torch.zeros(B2, dtype=torch.bool)
    mask = torch.zeros(B2, l, dtype=torch.bool)
    if training:
        s = s + s_noise * eps_s
        z = z + z_noise * eps_z
        if s_frac > 0:
            masked = u_s < s_frac
            s = torch.where(masked[:, None], repl, s)
        if z_frac > 0:
            span = (u_span * z_frac * l).long()
            start = (u_start * (l - span).clamp(min=1)).long()
            idx = torch.arange(l)[None]
            mask = (idx >= start[:, None]) & (idx < (start + span)[:, None])
            z = z.masked_fill(mask[:, None, :], 0.)
    return z, s, masked, mask


def run_perturb(dev, z, s, d, cfg, training):
    B2, E, l = z.shape
    S = s.shape[1]
    on = lambda t: None if t is None else t.to(dev)
    zb = z.permute(0, 2, 1).contiguous().to(dev)                 # frame-major storage: the kernel reads the permuted view
    outs = []
    for _ in range(2):
        zo, so = Fenced((B2, E, l), dev), Fenced((B2, S), dev)
        mk, ss = Fenced((B2,), dev, torch.uint8), Fenced((2 * B2,), dev, torch.int32)
        ops.latent_perturb(zb.permute(0, 2, 1), on(s), on(d.get("eps_z")), on(d.get("eps_s")), on(d.get("u_s")), on(d.get("repl")),
                           on(d.get("u_span")), on(d.get("u_start")), zo.t, so.t, mk.t, ss.t, *cfg, training)
        for f, name in ((zo, "z_out"), (so, "s_out"), (mk, "masked"), (ss, "start_span")):
            f.check(name)
        outs.append((zo, so, mk, ss))
    for a, b in zip(*outs):
        assert torch.equal(bits(a.t), bits(b.t)), "two launches differ"
    return outs[0]


def draws(B2, E, l, S, seed, s_mode):
    g = gen(seed)
    d = {"eps_s": torch.randn(B2, S, generator=g), "eps_z": torch.randn(B2, E, l, generator=g), "u_s": torch.rand(B2, generator=g),
         "repl": torch.randn(B2, S, generator=g), "u_span": torch.rand(B2, generator=g), "u_start": torch.rand(B2, generator=g)}
    # row 0: the span covers everything but one frame (frac 1: trunc(u l) = l - 1, start 0);  row 1: span 0, start at the last frame
    d["u_span"][0], d["u_start"][0] = ONE_MINUS, ONE_MINUS
    d["u_span"][1], d["u_start"][1] = 0.0, ONE_MINUS
    if s_mode == "all":
        d["u_s"].zero_()
    elif s_mode == "none":
        d["u_s"].fill_(ONE_MINUS)
    else:
        d["u_s"][0], d["u_s"][1] = 0.0, ONE_MINUS
    return d


@pytest.mark.parametrize("s_mode", ["mixed", "all", "none"])
@pytest.mark.parametrize("E,S", [(6, 16), (8, 32)])
@pytest.mark.parametrize("l", [1, 2, 38])
@pytest.mark.parametrize("B2", [2, 6])
def test_perturb(dev, B2, l, E, S, s_mode):
    g = gen(B2 * 1000 + l * 10 + E)
    z, s = torch.randn(B2, E, l, generator=g), torch.randn(B2, S, generator=g)
    d = draws(B2, E, l, S, 7 + B2 + l, s_mode)
    for z_frac, s_frac in ((1.0, 0.3), (0.25, 0.3), (0.0, 0.0)):
        cfg = (0.2, 0.3, s_frac, z_frac)
        zr, sr, masked, mask = perturb_ref(z, s, d["eps_z"], d["eps_s"], d["u_s"], d["repl"], d["u_span"], d["u_start"], *cfg, True)
        zo, so, mk, ss = run_perturb(dev, z, s, d, cfg, True)
        case = f"B2 {B2} l {l} E {E} S {S} {s_mode} z_frac {z_frac}"
        if z_frac == 1.0:       # the forced rows did what they were forced to
            assert int(mask[0].sum()) == l - 1 and not bool(mask[0, l - 1]), case
            assert int(mask[1].sum()) == 0 and ss.t.cpu()[2:4].tolist() == [l - 1, 0], case
        if s_frac > 0 and s_mode != "mixed":
            assert bool(masked.all()) == (s_mode == "all") and bool(masked.any()) == (s_mode == "all"), case
        st, sp = ss.t.cpu()[0::2].long(), ss.t.cpu()[1::2].long()
        idx = torch.arange(l)[None]
        got_mask = (idx >= st[:, None]) & (idx < (st + sp)[:, None])
        assert torch.equal(got_mask, mask), f"{case}: zeroed frames differ from the fp32 expression"
        assert torch.equal(mk.t.cpu().bool(), masked), f"{case}: replaced rows differ"
        assert torch.equal(zo.t.cpu() == 0, zr == 0), case
        assert within_one_ulp(zo.t, zr) and within_one_ulp(so.t, sr), f"{case}: more than 1 ulp"
        assert torch.equal(so.t.cpu()[masked], d["repl"][masked]), case
        # backward: exact
        dz_out, ds_out = torch.randn(B2, E, l, generator=g), torch.randn(B2, S, generator=g)
        want_dz = dz_out.masked_fill(mask[:, None, :], 0.)
        want_ds = torch.where(masked[:, None], 0., ds_out).view(B2 // 2, 2, S).flip(1).reshape(B2, S)
        prev = None
        for _ in range(2):
            dz, ds = Fenced((B2, E, l), dev), Fenced((B2, S), dev)
            ops.latent_perturb_bwd(dz_out.to(dev), ds_out.to(dev), mk.t, ss.t, dz.t, ds.t)
            dz.check("dz"), ds.check("ds")
            assert torch.equal(dz.t.cpu(), want_dz) and torch.equal(ds.t.cpu(), want_ds), f"{case}: backward"
            assert prev is None or (torch.equal(bits(prev[0]), bits(dz.t)) and torch.equal(bits(prev[1]), bits(ds.t)))
            prev = (dz.t, ds.t)


@pytest.mark.parametrize("B2,l,E,S", [(2, 1, 6, 16), (6, 38, 8, 32)])
def test_perturb_eval_only_swaps(dev, B2, l, E, S):
    g = gen(3)
    z, s = torch.randn(B2, E, l, generator=g), torch.randn(B2, S, generator=g)
    zo, so, mk, ss = run_perturb(dev, z, s, {}, (0.2, 0.2, 0.1, 0.25), False)
    assert torch.equal(zo.t.cpu(), z) and torch.equal(so.t.cpu(), s.view(B2 // 2, 2, S).flip(1).reshape(B2, S))
    assert not bool(mk.t.any()) and not bool(ss.t[1::2].any())


# ================================================================================================================ loss
def loss_inputs(B2, L, seed):
    g = gen(seed)
    logits = 2.0 * torch.randn(B2, 9, L, generator=g)
    chart = torch.rand(B2, 9, L, generator=g)
    r = torch.rand(B2, 7, L, generator=g)
    hits = chart[:, :7]
    hits[r < 0.3] = 0.0                       # exact 0 and 1 beside the soft values
    hits[r > 0.7] = 1.0
    big = torch.rand(B2, 7, L, generator=g)
    logits[:, :7][big < 0.05] = 40.0
    logits[:, :7][big > 0.95] = -40.0
    return logits, chart, torch.randn(B2, 5, generator=g) + 5, 10 * torch.rand(B2, 5, generator=g)


def loss_ref(logits, chart, pl, tl, masked, ema, first, training, s_reg, w_reg, seed):
    """fp64: components, sum |terms| / N per component, the EMA after the step, the loss, and d (seed * loss) / d (logits, labels)."""
    x, y = logits.double().requires_grad_(True), chart.double()
    p, t = pl.double().requires_grad_(True), tl.double()
    B2, _, L = x.shape
    th = y[:, :7]
    floor = -torch.special.xlogy(th, th) - torch.special.xlogy(1 - th, 1 - th)
    bce = F.binary_cross_entropy_with_logits(x[:, :7], th, reduction="none")
    comps = list((bce - floor).mean(dim=(0, 2)).unbind())
    scale = list(((bce.abs() + floor.abs()).sum(dim=(0, 2)) / (B2 * L)).detach().unbind())
    for n in range(3):
        c = F.mse_loss(x[:, 7:].diff(n=n), y[:, 7:].diff(n=n))
        comps.append(c)
        scale.append(c.detach())
    sq = (p - t).pow(2).mean(dim=1)
    lab = torch.where(masked, 0., sq).sum() / (~masked).sum().clamp(min=1)
    comps.append(lab)
    scale.append(lab.detach())
    losses = torch.stack(comps)
    ema = ema.double().clone()
    if training:
        ema = losses.detach().clone() if first else torch.lerp(ema, losses.detach(), 0.01)
    loss = (torch.tensor(WEIGHTS, dtype=torch.float64) * losses / ema.clamp(min=1e-8)).sum() + w_reg * s_reg
    (seed * loss).backward()
    return losses.detach(), torch.stack(scale), ema, loss.detach(), x.grad, p.grad


def run_loss(dev, logits, chart, pl, tl, masked, ema, flag, training, s_reg, w_reg, seed):
    B2, _, L = logits.shape
    d = lambda t: t.to(dev).contiguous()
    lg, ch, p, t = d(logits), d(chart), d(pl), d(tl)
    mk = d(masked.to(torch.uint8))
    sr, gs = torch.tensor([s_reg], dtype=torch.float32, device=dev), torch.tensor([seed], dtype=torch.float32, device=dev)
    res = []
    for _ in range(2):
        e = Fenced((11,), dev)
        e.t.copy_(ema)
        fl = Fenced((1,), dev, torch.uint8)
        fl.t.fill_(flag)
        out, coef, ws = Fenced((13,), dev), Fenced((11,), dev), Fenced((ops.latent_loss_ws_floats(B2, L),), dev)
        ops.latent_loss(lg, ch, p, t, mk, sr, e.t, fl.t, out.t, coef.t, ws.t, w_reg, training)
        dl, dlab, dsr = Fenced((B2, 9, L), dev), Fenced((B2, 5), dev), Fenced((1,), dev)
        ops.latent_loss_bwd(lg, ch, p, t, mk, coef.t, gs, dl.t, dlab.t, dsr.t, w_reg)
        for f, name in ((e, "loss_ema"), (fl, "flag"), (out, "out"), (coef, "coef"), (ws, "ws"), (dl, "dlogits"), (dlab, "dlabels"), (dsr, "ds_reg")):
            f.check(name)
        res.append((e, fl, out, coef, dl, dlab, dsr))
    for a, b in zip(*res):
        assert torch.equal(bits(a.t), bits(b.t)), "two launches differ"
    return [f.t.cpu() for f in res[0]]


def check_loss(dev, B2, L, masked, seed, modes=("first", "later", "eval")):
    T = ops.latent_loss_block_frames()
    logits, chart, pl, tl = loss_inputs(B2, L, seed)
    s_reg, w_reg, gseed = -7.3e-3, 1e-3, 0.7
    ema0 = 0.5 + torch.rand(11, generator=gen(seed + 1))
    for mode in modes:
        training, flag = mode != "eval", int(mode != "first")
        losses, scale, ema_ref, loss_ref_, dx, dp = loss_ref(logits, chart, pl, tl, masked, ema0, mode == "first", training, s_reg, w_reg, gseed)
        ema, fl, out, coef, dl, dlab, dsr = run_loss(dev, logits, chart, pl, tl, masked, ema0, flag, training, s_reg, w_reg, gseed)
        case = f"B2 {B2} L {L} {mode}"
        err = (out[:11].double() - losses).abs() / scale.clamp(min=1e-300)
        print(f"{case}: component errors / (sum |terms| / N) max {float(err.max()):.2e}")
        assert bool((err <= 2e-5).all()), (case, err)
        if bool(masked.all()):
            assert float(out[10]) == 0.0 and not bool(dlab.any()), f"{case}: all rows masked"
        # loss_ema and the flag
        if training:
            want = out[:11].double() if mode == "first" else torch.lerp(ema0.double(), out[:11].double(), 0.01)
            assert int(fl) == 1 and torch.allclose(ema.double(), want, rtol=1e-6, atol=0), case
        else:
            assert int(fl) == flag and torch.equal(ema, ema0), f"{case}: eval touched loss_ema"
        terms = torch.tensor(WEIGHTS, dtype=torch.float64) * out[:11].double() / ema.double().clamp(min=1e-8)
        assert abs(float(out[12]) - float(terms.sum() + w_reg * s_reg)) <= 1e-6 * float(terms.abs().sum() + abs(w_reg * s_reg)), case
        assert abs(float(out[12]) - float(loss_ref_)) <= 2e-5 * float(terms.abs().sum()), case
        assert float(out[11]) == float(torch.tensor(s_reg, dtype=torch.float32)) and abs(float(dsr) - gseed * w_reg) <= 1e-9, case
        # gradients, per channel
        for c in range(9):
            e = rel_l2(dl[:, c], dx[:, c])
            assert e <= 1e-5, (case, "dlogits channel", c, e)
        if bool((~masked).any()):
            for c in range(5):
                assert rel_l2(dlab[:, c], dp[:, c]) <= 1e-5, (case, "dlabels column", c)
        assert not bool(dlab[masked].any()), case
        # the cursor stencil, frame by frame at the ends of a row and around every tile boundary
        frames = {0, 1, 2, L - 3, L - 2, L - 1}
        for k in range(T, L + 2, T):
            frames |= {k - 2, k - 1, k, k + 1}
        frames = sorted(f for f in frames if 0 <= f < L)
        for c in (7, 8):
            rms = dx[:, c].pow(2).mean(-1, keepdim=True).sqrt()
            fe = ((dl[:, c].double() - dx[:, c]).abs() / rms)[:, frames]
            assert bool((fe <= 1e-5).all()), (case, "cursor frames", c, frames, fe.max())


def _lengths():
    T = 256          # od_latent_loss_block_frames(); test_loss_block_frames_constant holds the kernel to it
    return [3, 4, 5, T - 1, T, T + 1, T + 2, 2 * T + 3]


def test_loss_block_frames_constant(dev):
    assert ops.latent_loss_block_frames() == 256 and ops.latent_loss_ws_floats(6, 257) == 6 * 2 * 10


@pytest.mark.parametrize("L", _lengths())
@pytest.mark.parametrize("B2", [2, 6])
def test_loss(dev, B2, L):
    masked = torch.arange(B2) % 3 == 1 if B2 > 2 else torch.tensor([False, True])
    check_loss(dev, B2, L, masked, 100 + L)


@pytest.mark.parametrize("B2,L", [(2, 5), (6, 258)])
def test_loss_all_rows_masked(dev, B2, L):
    check_loss(dev, B2, L, torch.ones(B2, dtype=torch.bool), 300 + L)


@pytest.mark.parametrize("B2,L", [(2, 4), (6, 257)])
def test_loss_one_row_unmasked(dev, B2, L):
    masked = torch.ones(B2, dtype=torch.bool)
    masked[B2 - 1] = False
    check_loss(dev, B2, L, masked, 400 + L)


@pytest.mark.parametrize("B2,L", [(6, 300)])
def test_loss_none_masked(dev, B2, L):
    check_loss(dev, B2, L, torch.zeros(B2, dtype=torch.bool), 500, modes=("later",))


# ================================================================================================================ MMD
def mmd_ref(z, p):
    z = z.double().requires_grad_(True)
    p = p.double()
    n, d = z.shape

    def kernel(a, b):
        d2 = (a[:, None, :] - b[None, :, :]).pow(2).sum(-1)
        return sum(2. * d * s / (2. * d * s + d2) for s in SCALES)
    off = 1. - torch.eye(n, dtype=torch.float64)
    zz = (kernel(z, z) * off).sum() / (n * (n - 1))
    pp = (kernel(p, p) * off).sum() / (n * (n - 1))
    zp = kernel(z, p).mean()
    v = zz + pp - 2. * zp
    v.backward()
    return float(v.detach()), float(zz.detach()), float(pp.detach()), float(zp.detach()), z.grad


@pytest.mark.parametrize("N,D,twin", [(2, 16, False), (3, 32, False), (33, 32, False), (64, 32, False), (130, 32, False), (8, 32, True)])
def test_mmd(dev, N, D, twin):
    g = gen(N * 100 + D)
    z, p = torch.randn(N, D, generator=g) * 1.3 + 0.2, torch.randn(N, D, generator=g)
    if twin:
        z[5] = z[2]
    v, zz, pp, zp, dz_ref = mmd_ref(z, p)
    res = []
    for _ in range(2):
        out, dz, ws = Fenced((4,), dev), Fenced((N, D), dev), Fenced((3 * N,), dev)
        ops.mmd_imq(z.to(dev), p.to(dev), out.t, dz.t, ws.t)
        for f, name in ((out, "out"), (dz, "dz"), (ws, "ws")):
            f.check(name)
        res.append((out, dz))
    for a, b in zip(*res):
        assert torch.equal(bits(a.t), bits(b.t)), "two launches differ"
    out, dz = res[0][0].t.cpu(), res[0][1].t.cpu()
    verr, gerr = abs(float(out[0]) - v), rel_l2(dz, dz_ref)
    print(f"N {N} D {D}: value {float(out[0]):+.6e} (fp64 {v:+.6e}), error {verr:.2e} of bound {2e-5 * (abs(zz) + abs(pp) + 2 * abs(zp)):.2e}; "
          f"gradient rel L2 {gerr:.2e}")
    assert verr <= 2e-5 * (abs(zz) + abs(pp) + 2 * abs(zp))
    for got, want in zip(out[1:], (zz, pp, zp)):
        assert abs(float(got) - want) <= 2e-5 * abs(want)
    assert gerr <= 1e-3
    # the stored gradient under a seed: one fp32 product per element
    gs = torch.tensor([0.37], dtype=torch.float32, device=dev)
    y = Fenced((N, D), dev)
    ops.scale_by(res[0][1].t, gs, y.t)
    y.check("scale_by")
    assert torch.equal(y.t.cpu(), dz * torch.tensor(0.37, dtype=torch.float32))
