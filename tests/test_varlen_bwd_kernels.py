"""The varlen backward kernels of ragged training, on the emulator and on the MI355X (the `dev` fixture): od_flash_attn_bwd_varlen,
od_dwconv_bwd_varlen, od_uhead_bwd_varlen, od_uhead_tail_bwd_varlen, od_make_xt_varlen, od_loss_grad_varlen.

Layout: the padded (B, Lpad) frame layout; lens[b] (device int32) is sequence b's valid length.  Every padded row / frame of every input
is NaN (q, k, v, dout, x, dy, xt, x0, x1, the predicted v) — except o and lse, which the varlen forward's contract leaves as 0 there — and
every output is NaN-filled before the call: reading past a sequence's end, masking by a multiplication with zero or leaving an element
unwritten shows up as NaN.  Accumulated outputs (weight gradients, dsq, sums) are prefilled with finite values and must come out as
prefill + sum.  The reference is fp64 on each unpadded sequence alone.

Bounds.
  * attention: test_attention_paths.py's BOUNDS for the kernel pair (`grad`: block and global relative L2), per sequence, blocks of 64 rows.
    One exception, with its reason: at lens[b] = 1 the softmax has one key, P = 1 and dS = P (dP - delta) is exactly zero in the reference,
    so dq = dk = 0 there and a relative error has no denominator.  The kernel forms dP - delta from two fp32 sums of the same products in
    different orders; what is left is relative to the terms ls (|dP| + |delta|) |k| (|q|): those two are measured against that scale with
    BOUNDS' `terms` bound (the operand's unit roundoff), as that file does for its cancelling families.  dv = dO there and keeps `grad`.
  * everything else: test_step_paths.py's rule — the same restated formula evaluated in plain fp32 torch; its error against fp64 in the same
    metric, times 4, and never less than 8 fp32 eps, is the kernel's bound.  Sums are measured element by element against the sum of the
    absolute values of their terms; the conv's fixed-point block sums add their step 2^-41 per contribution.  A bf16 dx is the fp32 formula
    rounded to bf16 once.
  * outputs at padded rows / frames: exactly zero.
"""
import math

import pytest
import torch
import torch.nn.functional as F

from osu_dreamer_amd import det, ops
from kernel_backend import bits, dev  # noqa: F401
from test_attention_paths import BOUNDS, LN2, check_blocks, reference

LOG2E = math.log2(math.e)
NAN = float("nan")
EPS32 = float(torch.finfo(torch.float32).eps)
FLOOR = 8 * EPS32


def _lens_dev(lens, device):
    return torch.tensor(lens, dtype=torch.int32, device=device)


def held(what, out, ref, ref32, scale=None, extra_abs=0.0):
    """max over elements of |out - ref| / scale within max(4 x the fp32 evaluation's, 8 eps) (+ extra_abs / scale)."""
    out, ref, ref32 = out.detach().double().cpu(), ref.detach().double().cpu(), ref32.detach().double().cpu()
    den = (ref.abs() if scale is None else scale.detach().double().cpu()).clamp_min(1e-300)
    ek, e32 = ((out - ref).abs() / den), ((ref32 - ref).abs() / den)
    ek = torch.nan_to_num(ek, nan=float("inf"))
    bound = max(4 * float(e32.max()), FLOOR)
    lim = bound + extra_abs / den
    worst = float((ek / lim).max())
    print(f"MEASURED {what}: error {float(ek.max()):.3e}, fp32 torch {float(e32.max()):.3e}, bound {bound:.3e}")
    assert worst <= 1.0, f"{what}: error {float(ek.max()):.3e} is {worst:.2f} x the bound {bound:.3e} (fp32 torch {float(e32.max()):.3e})"


def held_l2(what, out, ref, ref32):
    """relative L2 over the whole tensor within max(4 x the fp32 evaluation's, 8 eps)."""
    out, ref, ref32 = out.detach().double().cpu(), ref.detach().double().cpu(), ref32.detach().double().cpu()
    n = float(ref.norm()) + 1e-300
    ek, e32 = float((out - ref).norm()) / n, float((ref32 - ref).norm()) / n
    ek = float("inf") if math.isnan(ek) else ek
    bound = max(4 * e32, FLOOR)
    print(f"MEASURED {what}: error {ek:.3e}, fp32 torch {e32:.3e}, bound {bound:.3e}")
    assert ek <= bound, f"{what}: relative L2 {ek:.3e} > {bound:.3e} (fp32 torch {e32:.3e})"


# ================================================================ attention backward
ATTN_CONFIGS = [(op, hd) for op in ("bf16", "fp32") for hd in (32, 64, 128)]
TORCH = {"bf16": torch.bfloat16, "fp32": torch.float32}


def attn_lens(Lpad):
    """one key; both sides of the 48-key wave of the hd-128 dK/dV kernel and of the 64-key tile; Lpad - 1 and Lpad."""
    return [1, 47, 48, 49, 63, 64, 65, Lpad - 1, Lpad]


def _attn_problem(op, hd, lens, Lpad, H, device, seed):
    """q (pre-multiplied), k, v, dout with NaN padded rows in the engine's layout; o, lse from the varlen forward (0 on padded rows)."""
    gen = torch.Generator().manual_seed(seed)
    B, dh, t = len(lens), H * hd, TORCH[op]
    scale = 1.0 / math.sqrt(hd)
    q = torch.randn(B, Lpad, dh, generator=gen) * 1.5 * (scale * LOG2E)
    k = torch.randn(B, Lpad, dh, generator=gen) * 1.5
    v = torch.randn(B, Lpad, dh, generator=gen)
    do = torch.randn(B, Lpad, dh, generator=gen)
    for b, Lb in enumerate(lens):
        for x in (q, k, v, do):
            x[b, Lb:] = NAN
    M = B * Lpad
    qk = torch.empty(M, 2 * dh, dtype=t, device=device)
    qkv = torch.full((M, 3 * dh), NAN, dtype=t, device=device)
    qk[:, :dh], qk[:, dh:], qkv[:, 2 * dh:] = (x.reshape(M, dh).to(t).to(device) for x in (q, k, v))
    q, k, v = qk[:, :dh], qk[:, dh:], qkv[:, 2 * dh:]
    do = do.reshape(M, dh).to(t).to(device)
    o = torch.full((M, dh), NAN, dtype=t, device=device)
    lse = torch.full((B, H, Lpad), NAN, device=device)
    lens_d = _lens_dev(lens, device)
    ops.flash_attn_fwd_varlen(q, k, v, o, lse, lens_d, B, H, Lpad, hd, scale, q_prescaled=True)
    for b, Lb in enumerate(lens):                            # the forward's contract, which the backward relies on
        assert torch.count_nonzero(o.reshape(B, Lpad, dh)[b, Lb:]).item() == 0 and torch.count_nonzero(lse[b, :, Lb:]).item() == 0
    return q, k, v, do, o, lse, lens_d, scale


def _attn_bwd(q, k, v, do, o, lse, lens_d, B, H, L, hd, scale):
    M, dh = B * L, H * hd
    dqk = torch.full((M, 2 * dh), NAN, dtype=q.dtype, device=q.device)
    dqkv = torch.full((M, 3 * dh), NAN, dtype=q.dtype, device=q.device)
    delta = torch.full((B, H, L), NAN, device=q.device)
    dq, dk, dv = dqk[:, :dh], dqk[:, dh:], dqkv[:, 2 * dh:]
    if lens_d is None:
        ops.flash_attn_bwd(q, k, v, o, do, lse, delta, dq, dk, dv, B, H, L, hd, scale, q_prescaled=True)
    else:
        ops.flash_attn_bwd_varlen(q, k, v, o, do, lse, delta, dq, dk, dv, lens_d, B, H, L, hd, scale, q_prescaled=True)
    assert bool(torch.isnan(dqkv[:, :2 * dh]).all()), "the backward wrote outside dv's columns"
    return dq, dk, dv


def _check_attn(op, hd, lens, Lpad, H, device, seed, alone=True):
    B, dh = len(lens), H * hd
    q, k, v, do, o, lse, lens_d, scale = _attn_problem(op, hd, lens, Lpad, H, device, seed)
    dq, dk, dv = _attn_bwd(q, k, v, do, o, lse, lens_d, B, H, Lpad, hd, scale)
    bnd = BOUNDS[op]
    r3 = lambda x: x.reshape(B, Lpad, dh)                     # noqa: E731
    hs = lambda x, Lb: x.reshape(Lb, H, hd).permute(1, 0, 2)  # noqa: E731  (Lb, H hd) -> (H, Lb, hd)
    for b, Lb in enumerate(lens):
        case = f"{op}-hd{hd}-Lpad{Lpad}-len{Lb}"
        for n, g in (("dq", dq), ("dk", dk), ("dv", dv)):
            pad = r3(g)[b, Lb:]
            assert torch.count_nonzero(pad).item() == 0 and not bool(torch.isnan(pad.float()).any()), f"{case}: {n} rows >= {Lb} are not exact zeros"
        sq, sk, sv, sdo, so = (hs(r3(x)[b, :Lb], Lb).double() for x in (q, k, v, do, o))
        if Lb == 1:       # (reference() ranks a row's two largest scores: it needs two keys.  One key: P = 1, so dq = dk = 0 and dv = dO)
            refs = [dict(dq=torch.zeros_like(sq[h]), dk=torch.zeros_like(sk[h]), dv=sdo[h]) for h in range(H)]
        else:
            refs = [reference(sq[h], sk[h], sv[h], sdo[h], LN2, True, so[h]) for h in range(H)]
        for n, g in (("dq", dq), ("dk", dk), ("dv", dv)):
            out = hs(r3(g)[b, :Lb], Lb)
            ref = torch.stack([r[n] for r in refs])
            if Lb == 1 and n in ("dq", "dk"):
                # one key: dS = P (dP - delta) = 0 exactly; the kernel's residue is relative to ls (|dP| + |delta|) |k| (|q|)
                other = sk if n == "dq" else sq
                terms = LN2 * ((sdo * sv).sum(-1, keepdim=True).abs() + (sdo * so).sum(-1, keepdim=True).abs()) * other.abs()
                assert float(ref.abs().max()) == 0.0
                check_blocks(case, n + "/terms", out, ref, bnd["terms"], scale=terms)
            else:
                check_blocks(case, n, out, ref, bnd["grad"])
        if alone:
            # the sequence alone through the dense entry point at L = lens[b]: the same kernel pair on the same tiles, bit for bit
            a = [r3(x)[b, :Lb].contiguous() for x in (q, k, v, do, o)]
            aq, ak, av = _attn_bwd(a[0], a[1], a[2], a[3], a[4], lse[b:b + 1, :, :Lb].contiguous(), None, 1, H, Lb, hd, scale)
            for n, g, s in (("dq", dq, aq), ("dk", dk, ak), ("dv", dv, av)):
                assert torch.equal(bits(r3(g)[b, :Lb].contiguous()), bits(s.contiguous())), f"{case}: {n} differs from the sequence alone"


@pytest.mark.parametrize("Lpad", [130, 193])
@pytest.mark.parametrize("op,hd", ATTN_CONFIGS, ids=[f"{o}-hd{h}" for o, h in ATTN_CONFIGS])
def test_attn_bwd_varlen(dev, op, hd, Lpad):
    _check_attn(op, hd, attn_lens(Lpad), Lpad, 2, dev, seed=hd + Lpad, alone=Lpad == 130)


@pytest.mark.parametrize("op,hd", ATTN_CONFIGS, ids=[f"{o}-hd{h}" for o, h in ATTN_CONFIGS])
def test_attn_bwd_varlen_full_lengths_equal_dense(dev, op, hd):
    """Every lens[b] == Lpad: od_flash_attn_bwd's result, bit for bit, under the deterministic mode."""
    B, H, Lpad = 2, 1, 130
    q, k, v, do, o, lse, lens_d, scale = _attn_problem(op, hd, [Lpad] * B, Lpad, H, dev, seed=3 * hd)
    try:
        det.force(True)
        a = _attn_bwd(q, k, v, do, o, lse, lens_d, B, H, Lpad, hd, scale)
        b = _attn_bwd(q, k, v, do, o, lse, None, B, H, Lpad, hd, scale)
    finally:
        det.force(None)
    for n, x, y in zip(("dq", "dk", "dv"), a, b):
        assert not bool(torch.isnan(x.float()).any()) and torch.equal(bits(x.contiguous()), bits(y.contiguous())), n


@pytest.mark.gpu
def test_attn_bwd_varlen_long():
    """Lpad = 2112 (33 key tiles, 11 key blocks of the bf16 dK/dV kernel): a full sequence, one that ends inside a tile, one of 65 frames."""
    if not torch.cuda.is_available():
        pytest.skip("no GPU is visible")
    from osu_dreamer_amd import _lib
    _lib._lib = None
    _lib.lib()
    _check_attn("bf16", 64, [2112, 1500, 65], 2112, 2, torch.device("cuda:0"), seed=11, alone=False)


# ================================================================ depthwise conv backward
def _dw_formula(x, dy, w, R, dt):
    """dx, dw, db of y = conv1d(x, w, groups=C, padding=R) on one sequence (1, C, Lb) by autograd, in dtype dt; + the sums of |terms|."""
    x, dy, w = x.to(dt).requires_grad_(True), dy.to(dt), w.to(dt).requires_grad_(True)
    C = x.shape[1]
    b = torch.zeros(C, dtype=dt, requires_grad=True)
    y = F.conv1d(x, w[:, None, :], b, padding=R, groups=C)
    dx, dw, db = torch.autograd.grad(y, (x, w, b), dy)
    return dx[0].T, dw, db


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("ksize", [3, 5, 9])
def test_dwconv_bwd_varlen(dev, dtype, ksize):
    gen = torch.Generator().manual_seed(ksize)
    R, C, Lpad = ksize // 2, 64, 96
    lens = [1, 2, 4, 5, 64, 65, Lpad]                      # 1 .. 4: shorter than the k = 9 halo; 64 | 65: the 64-frame run border
    B = len(lens)
    x = torch.randn(B, Lpad, C, generator=gen)
    dy = torch.randn(B, Lpad, C, generator=gen)
    for b, Lb in enumerate(lens):
        x[b, Lb:] = NAN
        dy[b, Lb:] = NAN
    x, dy = x.to(dtype), dy.to(dtype)
    w = torch.randn(C, ksize, generator=gen) * 0.5
    dw0, db0 = torch.randn(C, ksize, generator=gen), torch.randn(C, generator=gen)
    dx = torch.full((B * Lpad, C), NAN, dtype=dtype, device=dev)
    dw, db = dw0.clone().to(dev), db0.clone().to(dev)
    ops.dwconv_bwd_varlen(x.reshape(B * Lpad, C).to(dev), w.to(dev), dy.reshape(B * Lpad, C).to(dev), dx, dw, db, _lens_dev(lens, dev), B, Lpad, ksize)
    dx3 = dx.reshape(B, Lpad, C)
    rw, rb, rw32, rb32, aw, ab = (torch.zeros_like(t, dtype=d) for t, d in ((w, torch.float64), (db0, torch.float64), (w, torch.float32),
                                                                           (db0, torch.float32), (w, torch.float64), (db0, torch.float64)))
    for b, Lb in enumerate(lens):
        assert torch.count_nonzero(dx3[b, Lb:]).item() == 0, f"dx of sequence {b} is not zero on its padding"
        xs, ys = x[b, :Lb].T[None], dy[b, :Lb].T[None]
        rdx, sw, sb = _dw_formula(xs, ys, w, R, torch.float64)
        fdx, fw, fb = _dw_formula(xs, ys, w, R, torch.float32)
        _, tw, tb = _dw_formula(xs.abs(), ys.abs(), w.abs(), R, torch.float64)
        held_l2(f"dwconv_bwd k{ksize} len {Lb} dx", dx3[b, :Lb], rdx, fdx.to(dtype))
        rw += sw; rb += sb; rw32 += fw; rb32 += fb; aw += tw; ab += tb
    n = sum(lens)
    held(f"dwconv_bwd k{ksize} dw", dw, dw0.double() + rw, dw0 + rw32, scale=dw0.abs().double() + aw, extra_abs=n * 2.0 ** -41)
    held(f"dwconv_bwd k{ksize} db", db, db0.double() + rb, db0 + rb32, scale=db0.abs().double() + ab, extra_abs=n * 2.0 ** -41)


# ================================================================ u-head backward and tail backward
def _uhead_mean(xs, W):
    """xs: (E, Lb); the u_head stack (model.py:58-65) and its mean over the sequence's own frames."""
    w0, b0, w1, b1, w3, b3, w4, b4 = W
    E, U = w0.shape[0], w1.shape[0]
    z = F.conv1d(xs[None], w0[:, None, :], b0, padding=1, groups=E)
    z = F.silu(F.conv1d(z, w1[:, :, None], b1))
    z = F.conv1d(z, w3[:, None, :], b3, padding=1, groups=U)
    z = F.silu(F.conv1d(z, w4[:, :, None], b4))
    return z[0].mean(-1)


def _uhead_grads(xt, lens, W, dfm, dt):
    Wt = [t.to(dt).requires_grad_(True) for t in W]
    loss = sum((dfm[b].to(dt) * _uhead_mean(xt[b, :, :Lb].to(dt), Wt)).sum() for b, Lb in enumerate(lens))
    return torch.autograd.grad(loss, Wt)


@pytest.mark.parametrize("U", [8, 32])
def test_uhead_bwd_varlen(dev, U):
    gen = torch.Generator().manual_seed(U)
    E, Lpad = 6, 122
    lens = [1, 2, 29, 30, 31, 60, 61, 120, 121, Lpad]        # window borders (30 owned frames), the 4-window block border (120), one frame
    B = len(lens)
    W = [torch.randn(E, 3, generator=gen) * 0.5, torch.randn(E, generator=gen) * 0.1, torch.randn(U, E, generator=gen) * 0.4,
         torch.randn(U, generator=gen) * 0.1, torch.randn(U, 3, generator=gen) * 0.5, torch.randn(U, generator=gen) * 0.1,
         torch.randn(U, U, generator=gen) * 0.2, torch.randn(U, generator=gen) * 0.1]
    xt = torch.randn(B, E, Lpad, generator=gen)
    for b, Lb in enumerate(lens):
        xt[b, :, Lb:] = NAN
    dfm = torch.randn(B, U, generator=gen)
    G0 = [torch.randn(t.shape, generator=gen) * 0.1 for t in W]
    G = [g.clone().to(dev) for g in G0]
    ops.uhead_bwd_varlen(xt.to(dev), [t.to(dev) for t in W], dfm.to(dev), G, _lens_dev(lens, dev), U)
    ref = _uhead_grads(xt, lens, W, dfm, torch.float64)
    r32 = _uhead_grads(xt, lens, W, dfm, torch.float32)
    for name, g, g0, r, f in zip(("w0", "b0", "w1", "b1", "w3", "b3", "w4", "b4"), G, G0, ref, r32):
        # a sum over frames and sequences through two SiLUs: measured against the tensor's own norm (its terms are not separable by autograd)
        held_l2(f"uhead_bwd U{U} d{name}", g.cpu().double() - g0.double(), r, f)


def _tail(fsum, mod, w, bo, lens, u_scale):
    U = fsum.shape[1]
    f = fsum / torch.tensor(lens, dtype=fsum.dtype)[:, None]
    fm = f * (1 + mod[:, :U]) + mod[:, U:]
    return u_scale * F.softplus(fm @ w + bo), f


def test_uhead_tail_bwd_varlen(dev):
    gen = torch.Generator().manual_seed(2)
    U, Lpad, u_scale = 32, 96, 3.4641
    lens = [1, 2, 29, 30, 64, 65, Lpad]
    B = len(lens)
    fsum = torch.randn(B, U, generator=gen) * torch.tensor(lens)[:, None]
    mod = torch.randn(B, 2 * U, generator=gen) * 0.2
    w, bo = torch.randn(U, generator=gen) * 0.3, torch.randn(1, generator=gen) * 0.1
    du = torch.randn(B, generator=gen)
    dw0, db0 = torch.randn(U, generator=gen), torch.randn(1, generator=gen)
    dfm, dmod = torch.full((B, U), NAN, device=dev), torch.full((B, 2 * U), NAN, device=dev)
    dw, db = dw0.clone().to(dev), db0.clone().to(dev)
    ops.uhead_tail_bwd_varlen(fsum.to(dev), mod.to(dev), w.to(dev), bo.to(dev), du.to(dev), dfm, dmod, dw, db, _lens_dev(lens, dev), Lpad, u_scale)

    def grads(dt):
        fs, m, ww, bb = (t.to(dt).requires_grad_(True) for t in (fsum, mod, w, bo))
        u, f = _tail(fs, m, ww, bb, lens, u_scale)
        f.retain_grad()
        (u * du.to(dt)).sum().backward()
        return f.grad, m.grad, ww.grad, bb.grad
    (rf, rm, rw, rb), (ff, fm_, fw, fb) = grads(torch.float64), grads(torch.float32)
    held("uhead_tail_bwd dfm", dfm, rf, ff)
    held("uhead_tail_bwd dmod", dmod, rm, fm_)
    held_l2("uhead_tail_bwd dw", dw.cpu().double() - dw0.double(), rw, fw)
    held_l2("uhead_tail_bwd db", db.cpu().double() - db0.double(), rb, fb)


# ================================================================ make_xt, loss_grad
def _ragged(B, E, Lpad, lens, gen):
    x = torch.randn(B, E, Lpad, generator=gen)
    for b, Lb in enumerate(lens):
        x[b, :, Lb:] = NAN
    return x


def test_make_xt_varlen(dev):
    gen = torch.Generator().manual_seed(4)
    E, Lpad = 6, 300
    lens = [1, 2, 42, 43, 255, 256, 257, Lpad]               # E Lb on both sides of the 256-thread block
    B = len(lens)
    x0, x1 = _ragged(B, E, Lpad, lens, gen), _ragged(B, E, Lpad, lens, gen)
    t = torch.tensor([0.0, 1.0, 0.3, 0.49999, 0.5, 0.7, 0.05, 0.95])
    dsq0 = torch.randn(B, generator=gen)
    xt = torch.full((B, E, Lpad), NAN, device=dev)
    dsq = dsq0.clone().to(dev)
    ops.make_xt_varlen(x0.to(dev), x1.to(dev), t.to(dev), xt, dsq, _lens_dev(lens, dev))
    for b, Lb in enumerate(lens):
        assert torch.count_nonzero(xt[b, :, Lb:]).item() == 0, f"xt of sequence {b} is not zero on its padding"

        def f(dt):
            a, e, w = x0[b, :, :Lb].to(dt), x1[b, :, :Lb].to(dt), t[b].to(dt)
            v = torch.lerp(a, e, w)
            return v, (v - e).square().sum(0).mean()
        (rv, rd), (fv, fd) = f(torch.float64), f(torch.float32)
        # lerp's two forms cancel: measured against |x0| + |x1|
        held(f"make_xt len {Lb} xt", xt[b, :, :Lb], rv, fv, scale=x0[b, :, :Lb].abs().double() + x1[b, :, :Lb].abs().double())
        held(f"make_xt len {Lb} dsq", dsq[b], dsq0[b].double() + rd, dsq0[b] + fd, scale=dsq0[b].abs().double() + rd)


def test_loss_grad_varlen(dev):
    gen = torch.Generator().manual_seed(6)
    E, Lpad, c0, osl_w, del_w = 6, 300, 0.0065, 1.0, 30.0
    lens = [1, 2, 42, 43, 255, 256, 257, Lpad]
    B = len(lens)
    xt, x1, v = (_ragged(B, E, Lpad, lens, gen) for _ in range(3))
    u = torch.rand(B, generator=gen) + 0.2
    dsq = torch.rand(B, generator=gen) * 4
    sums0 = torch.randn(B, 3, generator=gen)
    dv = torch.full((B, E, Lpad), NAN, device=dev)
    sums = sums0.clone().to(dev)
    ops.loss_grad_varlen(xt.to(dev), x1.to(dev), u.to(dev), v.to(dev), dsq.to(dev), dv, sums, _lens_dev(lens, dev), c0, osl_w, del_w)
    for b, Lb in enumerate(lens):
        assert torch.count_nonzero(dv[b, :, Lb:]).item() == 0, f"dv of sequence {b} is not zero on its padding"

        def f(dt):
            """train.py:89-101 on sequence b alone, its share 1 / B of the batch mean; + the sums of |terms| (fp64 only)."""
            xv, e, ub, d = xt[b, :, :Lb].to(dt), x1[b, :, :Lb].to(dt), u[b].to(dt).requires_grad_(True), dsq[b].to(dt)
            vv = v[b, :, :Lb].to(dt).requires_grad_(True)
            den = d + torch.tensor(c0, dtype=dt)
            r1, r2 = xv - ub * vv - e, vv - (xv - e) / den.sqrt()
            s1, s2 = r1.square().sum(0).mean(), r2.square().sum(0).mean()
            ds1du, = torch.autograd.grad(s1, ub, retain_graph=True)
            g, = torch.autograd.grad((osl_w * s1 / den + del_w * s2) / B, vv)
            terms = (2.0 / Lb) * ((osl_w / (B * den)) * r1.abs() * ub.abs() + (del_w / B) * r2.abs())
            return g, torch.stack([s1, s2, ds1du]).detach(), terms.detach(), (2.0 / Lb) * (r1 * vv).abs().sum().detach()
        (rg, rs, tg, t3), (fg, fs, _, _) = f(torch.float64), f(torch.float32)
        held(f"loss_grad len {Lb} dv", dv[b, :, :Lb], rg, fg, scale=tg)
        sc = sums0[b].abs().double() + torch.stack([rs[0], rs[1], t3])
        held(f"loss_grad len {Lb} sums", sums[b], sums0[b].double() + rs, sums0[b] + fs, scale=sc)
