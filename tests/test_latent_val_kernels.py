"""The kernels of the batched validation of LatentTrainer (od_replicate_tail in csrc/misc.hip; od_mmd_imq_pairs, od_latent_loss_maps and
od_latent_eval_maps in csrc/latent.hip) against the calls they stand for and against fp64.

Bounds:
  replicate tail   equal to F.pad(mode="replicate") per row, bit for bit; nothing outside [lens, plens) written
  MMD pairs        bit-equal to od_mmd_imq(N = 2) on each pair of rows
  loss per map     all 13 values bit-equal to od_latent_loss(training = 0) on the map's two rows copied out contiguously; loss_ema unchanged
  eval per map     every sum within 2e-5 of sum |terms| of the fp64 evaluation of eval_metrics' formulas (latent/train.py:210-255 of the
                   reference, restated here) on the same inputs: the bound of the latent backward tests for sums over frames; the two
                   means and z_var_min within 2e-5 relative
Every buffer is NaN-fenced, the padding behind every row's length holds NaN (so a load past a length poisons the result), and every
kernel is launched twice and must give the same bits.
"""
import pytest
import torch
import torch.nn.functional as F

from osu_dreamer_amd import _lib, ops
from kernel_backend import Flat, bits, dev  # noqa: F401

NAN = float("nan")
HALF_LENS = (306, 256, 27)       # per map: two tiles with a ragged second one, exactly one tile, under one tile (tiles of 256 frames)


def gen(seed):
    return torch.Generator().manual_seed(seed)


def i32(v, dev):
    return torch.tensor(v, dtype=torch.int32, device=dev)


def ragged(rows, C, Lmax, lens, g, dev, scale=1.0, uniform=False):
    """(rows, C, Lmax) on the CPU and its NaN-fenced device copy: row r random for lens[r] frames, NaN behind them."""
    x = torch.rand(rows, C, Lmax, generator=g) if uniform else scale * torch.randn(rows, C, Lmax, generator=g)
    for r, n in enumerate(lens):
        x[r, :, n:] = NAN
    return x, Flat((rows, C, Lmax), dev, fill=x)


def twice(run):
    a, b = run(), run()
    for x, y in zip(a, b):
        assert torch.equal(bits(x.contiguous()), bits(y.contiguous())), "two launches differ"
    return a


# ================================================================================================================ replicate tail
def test_replicate_tail(dev):
    N, C, Lpad = 3, 9, 40
    lens, plens = (40, 23, 1), (40, 36, 18)
    x, _ = ragged(N, C, Lpad, lens, gen(1), "cpu")

    def run():
        f = Flat((N, C, Lpad), dev, fill=x)
        ops.replicate_tail(f.v, i32(lens, dev), i32(plens, dev))
        assert bool(torch.isnan(f.buf[:64]).all() & torch.isnan(f.buf[64 + f.n:]).all()), "written outside the batch"
        return (f.v.cpu(),)
    got, = twice(run)
    for n in range(N):
        want = F.pad(x[n:n + 1, :, :lens[n]], (0, plens[n] - lens[n]), mode="replicate")[0]
        assert torch.equal(bits(got[n, :, :plens[n]]), bits(want)), f"row {n}: not the replicate padding"
        assert bool(torch.isnan(got[n, :, plens[n]:]).all()), f"row {n}: written at or past plens"


def test_replicate_tail_refusals(dev):
    N, C, Lpad = 4, 2, 12
    x = torch.rand(N, C, Lpad, generator=gen(2))
    f = Flat((N, C, Lpad), dev, fill=x)
    lens, plens = i32((0, 5, 12, 7), dev), i32((4, 13, 12, 3), dev)       # lens < 1; plens > Lpad; no tail; plens < lens
    ops.replicate_tail(f.v, lens, plens)
    got = f.v.cpu()
    assert bool(torch.isnan(got[:2]).all()) and torch.equal(got[2:], x[2:])
    assert bool(torch.isnan(f.buf[:64]).all() & torch.isnan(f.buf[64 + f.n:]).all())
    call = _lib.lib().od_replicate_tail
    for args in ((None, lens.data_ptr(), plens.data_ptr(), N, C, Lpad), (f.v.data_ptr(), None, plens.data_ptr(), N, C, Lpad),
                 (f.v.data_ptr(), lens.data_ptr(), None, N, C, Lpad), (f.v.data_ptr(), lens.data_ptr(), plens.data_ptr(), 0, C, Lpad),
                 (f.v.data_ptr(), lens.data_ptr(), plens.data_ptr(), N, 0, Lpad), (f.v.data_ptr(), lens.data_ptr(), plens.data_ptr(), N, C, 0)):
        with pytest.raises(_lib.HipKernelError, match="od_replicate_tail"):
            call(*args, 0)


# ================================================================================================================ MMD per pair
def test_mmd_pairs(dev):
    G, S = 3, 16
    g = gen(3)
    s, p = (torch.randn(2 * G, S, generator=g) * 1.3 + 0.2).to(dev), torch.randn(2 * G, S, generator=g).to(dev)

    def run():
        out, ws = Flat((G, 4), dev), Flat((6 * G,), dev)
        ops.mmd_imq_pairs(s, p, out.v, ws.v)
        out.check("pairs", "out"), ws.check("pairs", "ws")
        return (out.v.cpu(),)
    got, = twice(run)
    for i in range(G):
        out, dz, ws = Flat((4,), dev), Flat((2, S), dev), Flat((6,), dev)
        ops.mmd_imq(s[2 * i:2 * i + 2].contiguous(), p[2 * i:2 * i + 2].contiguous(), out.v, dz.v, ws.v)
        assert torch.equal(bits(got[i]), bits(out.v.cpu())), f"pair {i}: {got[i].tolist()} against od_mmd_imq's {out.v.tolist()}"


# ================================================================================================================ loss per map
def loss_inputs(dev):
    G, Hmax = len(HALF_LENS), max(HALF_LENS)
    g = gen(4)
    hl = [n for n in HALF_LENS for _ in range(2)]
    logits, lf = ragged(2 * G, 9, Hmax, hl, g, dev, scale=2.0)
    chart, cf = ragged(2 * G, 9, Hmax, hl, g, dev, uniform=True)
    r = torch.rand(2 * G, 7, Hmax, generator=g)
    hits = chart[:, :7]
    hits[(r < 0.3) & ~torch.isnan(hits)] = 0.0          # exact 0 and 1 beside the soft targets
    hits[(r > 0.7) & ~torch.isnan(hits)] = 1.0
    cf.v.copy_(chart)
    pl, tl = torch.randn(2 * G, 5, generator=g) + 5, 10 * torch.rand(2 * G, 5, generator=g)
    mmd = torch.randn(G, 4, generator=g) * 1e-2          # s_reg is its first column: element stride 4
    ema = 0.5 + torch.rand(11, generator=g)
    return hl, logits, lf, chart, cf, pl.to(dev), tl.to(dev), mmd.to(dev), ema.to(dev)


def test_loss_maps(dev):
    G, Hmax, w_reg = len(HALF_LENS), max(HALF_LENS), 1e-3
    hl, logits, lf, chart, cf, pl, tl, mmd, ema = loss_inputs(dev)
    ema0 = ema.clone()

    def run():
        out, ws = Flat((G, 13), dev), Flat((ops.latent_loss_ws_floats(2 * G, Hmax),), dev)
        ops.latent_loss_maps(lf.v, cf.v, i32(hl, dev), pl, tl, mmd[:, 0], ema, out.v, ws.v, w_reg)
        out.check("loss maps", "out")
        assert bool(torch.isnan(ws.buf[:64]).all() & torch.isnan(ws.buf[64 + ws.n:]).all()), "written outside ws"
        return (out.v.cpu(),)
    got, = twice(run)
    assert torch.equal(ema, ema0), "loss_ema was written"
    zero = torch.zeros(2, dtype=torch.uint8, device=dev)
    for i, L in enumerate(HALF_LENS):
        rows = slice(2 * i, 2 * i + 2)
        out, coef, ws = Flat((13,), dev), Flat((11,), dev), Flat((ops.latent_loss_ws_floats(2, L),), dev)
        flag = torch.ones(1, dtype=torch.uint8, device=dev)
        ops.latent_loss(logits[rows, :, :L].contiguous().to(dev), chart[rows, :, :L].contiguous().to(dev), pl[rows].contiguous(),
                        tl[rows].contiguous(), zero, mmd[i, :1].contiguous(), ema, flag, out.v, coef.v, ws.v, w_reg, False)
        want = out.v.cpu()
        assert torch.equal(bits(got[i]), bits(want)), f"map {i} (half length {L}): {got[i].tolist()} against od_latent_loss's {want.tolist()}"


def test_loss_maps_refuses_a_bad_pair(dev):
    G, Hmax = len(HALF_LENS), max(HALF_LENS)
    hl, _, lf, _, cf, pl, tl, mmd, ema = loss_inputs(dev)
    hl[2], hl[4], hl[5] = hl[2] - 1, 2, 2                 # map 1: the halves differ; map 2: under three frames
    out, ws = Flat((G, 13), dev), Flat((ops.latent_loss_ws_floats(2 * G, Hmax),), dev)
    ops.latent_loss_maps(lf.v, cf.v, i32(hl, dev), pl, tl, mmd[:, 0], ema, out.v, ws.v, 1e-3)
    got = out.v.cpu()
    assert not bool(torch.isnan(got[0]).any()) and bool(torch.isnan(got[1:]).all())


# ================================================================================================================ eval per map
def eval_ref(chart, pred, P, z, zl, pl, tl):
    """eval_metrics' formulas in fp64 on one map: the eight values and, for the five sums, sum |terms|."""
    x, p = chart[:, :P].double(), pred[:, :P].double()
    t0, p0 = x[0], p[0]
    px = torch.tensor([512., 384.], dtype=torch.float64)[:, None]
    txy, pxy = x[7:9] * px, p[7:9] * px
    tv, pv = txy.diff(dim=-1), pxy.diff(dim=-1)
    res, tot = (pv - tv).pow(2), (tv - tv.mean(dim=-1, keepdim=True)).pow(2)
    vals = [t0.mul(t0).sum(), p0.mul(t0).sum(), p0.mul(p0).sum(), res.sum(), tot.sum(), (pxy - txy).abs().mean(),
            (pl.double() - tl.double()).abs().mean(), z[:, :zl].double().var(dim=1).min()]
    mags = [t0.mul(t0).sum(), p0.mul(t0).abs().sum(), p0.mul(p0).sum(), res.sum(), tot.sum()]
    return [float(v) for v in vals], [float(m) for m in mags]


def test_eval_maps(dev):
    G, E = len(HALF_LENS), 8
    P = [2 * n for n in HALF_LENS]
    zl = [68, 57, 6]
    Pmax, lmax = max(P), max(zl)
    g = gen(5)
    chart, cf = ragged(G, 9, Pmax, P, g, dev, uniform=True)
    pred, pf = ragged(G, 9, Pmax, P, g, dev, uniform=True)
    chart[:, 7:9] = torch.cumsum(0.02 * torch.randn(G, 2, Pmax, generator=g), dim=-1) + 0.5      # a cursor that walks
    pred[:, 7:9] = chart[:, 7:9] + 0.05 * torch.randn(G, 2, Pmax, generator=g)
    for i, n in enumerate(P):
        chart[i, :, n:], pred[i, :, n:] = NAN, NAN
    cf.v.copy_(chart), pf.v.copy_(pred)
    z, zf = ragged(G, E, lmax, zl, g, dev)
    z[:, 3] = z[:, 3] * 0.1 + 2.0                          # the channel of least variance, far from zero mean
    for i, n in enumerate(zl):
        z[i, :, n:] = NAN
    zf.v.copy_(z)
    pl, tl = torch.randn(G, 5, generator=g) + 5, 10 * torch.rand(G, 5, generator=g)

    def run():
        out, ws = Flat((G, 8), dev), Flat((ops.latent_eval_maps_ws_floats(G, Pmax),), dev)
        ops.latent_eval_maps(cf.v, pf.v, i32(P, dev), zf.v, i32(zl, dev), pl.to(dev), tl.to(dev), out.v, ws.v)
        out.check("eval maps", "out")
        assert bool(torch.isnan(ws.buf[:64]).all() & torch.isnan(ws.buf[64 + ws.n:]).all()), "written outside ws"
        return (out.v.cpu(),)
    got, = twice(run)
    names = ("sum t^2", "sum p t", "sum p^2", "velocity residual", "velocity total", "cursor_px_mae", "label_mae", "z_var_min")
    for i in range(G):
        vals, mags = eval_ref(chart[i], pred[i], P[i], z[i], zl[i], pl[i], tl[i])
        for k, name in enumerate(names):
            bound = 2e-5 * (mags[k] if k < 5 else abs(vals[k]))
            err = abs(float(got[i, k]) - vals[k])
            print(f"map {i} {name}: {float(got[i, k]):.7g} (fp64 {vals[k]:.7g}), error {err:.2e} of bound {bound:.2e}")
            assert err <= bound, (i, name, float(got[i, k]), vals[k])


def test_eval_maps_refuses_bad_lengths(dev):
    G, E, Pmax, lmax = 3, 4, 20, 5
    g = gen(6)
    c, p, z = torch.rand(G, 9, Pmax, generator=g).to(dev), torch.rand(G, 9, Pmax, generator=g).to(dev), torch.randn(G, E, lmax, generator=g).to(dev)
    lab = torch.rand(G, 5, generator=g).to(dev)
    out, ws = Flat((G, 8), dev), Flat((ops.latent_eval_maps_ws_floats(G, Pmax),), dev)
    ops.latent_eval_maps(c, p, i32((20, 21, 18), dev), z, i32((5, 5, 6), dev), lab, lab, out.v, ws.v)
    got = out.v.cpu()
    assert not bool(torch.isnan(got[0]).any()) and bool(torch.isnan(got[1:]).all())
