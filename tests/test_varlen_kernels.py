"""The varlen (per-sequence valid length) kernels of the batched sampler, on the emulator and on the MI355X (the `dev` fixture).

Layout: the padded (B, Lpad) frame layout, rows b * Lpad + l; lens[b] (device int32) is sequence b's valid length.  Every padded row /
frame of every input is NaN, so anything that reads past a sequence's end, or masks by multiplying with zero, shows up as NaN.  Checks:
  * attention forward, every (dtype, head_dim) od_flash_attn_fwd accepts, Lpad on both sides of the fwd16x / fwd32 and NQT = 1 / 2 switches:
    valid rows against a dense fp64 masked softmax (test_attention_paths.py's bounds), rows >= lens[b] exactly 0, and each sequence bit for bit
    the non-varlen entry point run on that sequence alone at L = lens[b] whenever the dispatch picks the same kernel for both;
  * depthwise conv and u-head against torch on each unpadded sequence (and the conv bit for bit against od_dwconv on it);
  * grouped eta bit for bit od_sampler_eta on each group alone; the varlen step against the same step per song.
"""
import math

import pytest
import torch
import torch.nn.functional as F

from osu_dreamer_amd import ops
from kernel_backend import dev, rel_l2  # noqa: F401
from test_attention_paths import BOUNDS, EMU_MIN_L, FWD_CONFIGS, GPU_MIN_L, OPS, fwd_path

LOG2E = math.log2(math.e)
NAN = float("nan")


def _lens_for(Lpad):
    return [1, 63, 64, 65, Lpad - 1, Lpad]


def _on_gpu(device):
    return device.type == "cuda"


# ---------------------------------------------------------------- attention forward
# (Lpad, H): emulator 120 | 130 straddles its fwd16x switch (128); the GPU adds 2047 | 2112 around 2048 and, with H = 22, B H ceil(L / 128) =
# 6 x 22 x 17 = 2244 >= 2048 workgroups: the fp32 32-query form (NQT = 2; B = 1 alone runs the 16-query form)
EMU_SHAPES = [(120, 2), (130, 2)]
GPU_SHAPES = [(130, 2), (2047, 2), (2112, 22)]


def _attn_inputs(op, hd, pre, lens, Lpad, H, device, gen):
    B = len(lens)
    dh = H * hd
    q = torch.randn(B, Lpad, dh, generator=gen) * 1.5
    k = torch.randn(B, Lpad, dh, generator=gen) * 1.5
    v = torch.randn(B, Lpad, dh, generator=gen)
    scale = 1.0 / math.sqrt(hd)
    if pre:
        q = q * (scale * LOG2E)
    for b, Lb in enumerate(lens):
        q[b, Lb:] = NAN
        k[b, Lb:] = NAN
        v[b, Lb:] = NAN
    t = OPS[op]
    q, k, v = (x.reshape(B * Lpad, dh).to(t).to(device) for x in (q, k, v))
    return q, k, v, scale


def _attn_run(op, hd, pre, q, k, v, scale, B, H, L, lens_dev=None):
    dh = H * hd
    o = torch.full((B * L, dh), NAN, dtype=torch.bfloat16 if op == "f16" else q.dtype, device=q.device)
    lse = torch.full((B, H, L), NAN, dtype=torch.float32, device=q.device)
    if lens_dev is None:
        ops.flash_attn_fwd(q, k, v, o, lse, B, H, L, hd, scale, x3=(op == "x3"), q_prescaled=pre)
    else:
        ops.flash_attn_fwd_varlen(q, k, v, o, lse, lens_dev, B, H, L, hd, scale, x3=(op == "x3"), q_prescaled=pre)
    return o, lse


def _ref(qh, kh, vh, ls):
    """fp64 softmax attention of one (sequence, head): (Lb, hd) each."""
    s = ls * (qh @ kh.T)
    lse = torch.logsumexp(s, dim=1)
    o = torch.softmax(s, dim=1) @ vh
    mag = (ls * (qh.abs() @ kh.abs().T)).max(dim=1).values
    return o, lse, mag


# test_attention_paths.py's configurations plus the pre-multiplied-q forms the engine runs (it always passes q_prescaled): fp32-as-3-x-bf16
# (the sampler's compliant mode), and head_dim 32 in bf16 / fp32
VARLEN_CONFIGS = FWD_CONFIGS + [c for c in (("x3", 64, True), ("x3", 32, True), ("bf16", 32, True), ("fp32", 32, True)) if c not in FWD_CONFIGS]


@pytest.mark.parametrize("op,hd,pre", VARLEN_CONFIGS, ids=[f"{o}-hd{h}-{'pre' if p else 'raw'}" for o, h, p in VARLEN_CONFIGS])
def test_attn_fwd_varlen(dev, op, hd, pre):
    gpu = _on_gpu(dev)
    gen = torch.Generator().manual_seed(hd * 7 + len(op) + pre)
    min_l = GPU_MIN_L if gpu else EMU_MIN_L
    bnd = BOUNDS[op]
    for Lpad, H in (GPU_SHAPES if gpu else EMU_SHAPES):
        lens = _lens_for(Lpad)
        B = len(lens)
        q, k, v, scale = _attn_inputs(op, hd, pre, lens, Lpad, H, dev, gen)
        lens_dev = torch.tensor(lens, dtype=torch.int32, device=dev)
        o, lse = _attn_run(op, hd, pre, q, k, v, scale, B, H, Lpad, lens_dev)
        dh = H * hd
        o3 = o.reshape(B, Lpad, dh)
        ls = math.log(2.0) if pre else scale
        batch_path = fwd_path(op, hd, pre, B, H, Lpad, min_l=min_l)
        heads = range(H) if H <= 2 else (0, H // 2, H - 1)
        for b, Lb in enumerate(lens):
            # padded query rows: exactly zero, o and lse
            assert torch.count_nonzero(o3[b, Lb:]).item() == 0, (Lpad, Lb)
            assert torch.count_nonzero(lse[b, :, Lb:]).item() == 0, (Lpad, Lb)
            q3, k3, v3 = (x.reshape(B, Lpad, dh)[b, :Lb] for x in (q, k, v))
            for h in heads:
                sl = slice(h * hd, (h + 1) * hd)
                ro, rl, mag = _ref(q3[:, sl].double(), k3[:, sl].double(), v3[:, sl].double(), ls)
                err = rel_l2(o3[b, :Lb, sl].double(), ro)
                assert err <= bnd["o"][0], (op, hd, pre, Lpad, Lb, h, err)
                a, r = bnd["lse"]
                dl = (lse[b, h, :Lb].double() - rl).abs()
                assert bool((dl <= a + r * mag).all()), (op, hd, pre, Lpad, Lb, h, float(dl.max()))
            # the sequence alone through the non-varlen entry point: bit for bit when the dispatch picks the same kernel
            if fwd_path(op, hd, pre, 1, H, Lb, min_l=min_l) == batch_path:
                so, slse = _attn_run(op, hd, pre, q3.contiguous(), k3.contiguous(), v3.contiguous(), scale, 1, H, Lb)
                assert torch.equal(o3[b, :Lb].view(torch.int16) if o.dtype != torch.float32 else o3[b, :Lb].view(torch.int32),
                                   so.view(torch.int16) if so.dtype != torch.float32 else so.view(torch.int32)), (op, hd, pre, Lpad, Lb)
                assert torch.equal(lse[b, :, :Lb].view(torch.int32), slse[0].view(torch.int32)), (op, hd, pre, Lpad, Lb)


# ---------------------------------------------------------------- depthwise conv
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("ksize", [3, 5])
def test_dwconv_varlen(dev, dtype, ksize):
    gen = torch.Generator().manual_seed(ksize)
    R = ksize // 2
    # (Lpad, copies of the length set, C).  od_dwconv takes its RUN = 32 form from B (C / 8) ceil(L / 32) >= OD_DW_SMALL_THREADS: 10 on the
    # emulator (both shapes), 131072 on the GPU — there 48 x 64 x 47 = 144384 (the 48 sequences of length <= 1500, C = 512) reaches it
    shapes = [(70, 1, 64), (200, 1, 64)] if not _on_gpu(dev) else [(70, 1, 64), (1500, 8, 512)]
    for Lpad, reps, C in shapes:
        lens = _lens_for(Lpad) * reps
        B = len(lens)
        x = torch.randn(B, Lpad, C, generator=gen)
        for b, Lb in enumerate(lens):
            x[b, Lb:] = NAN
        x = x.to(dtype)
        w = torch.randn(C, ksize, generator=gen) * 0.5
        bias = torch.randn(C, generator=gen) * 0.1
        xd = x.reshape(B * Lpad, C).to(dev)
        y = torch.full((B * Lpad, C), NAN, dtype=dtype, device=dev)
        ops.dwconv_varlen(xd, w.to(dev), bias.to(dev), y, torch.tensor(lens, dtype=torch.int32, device=dev), B, Lpad, ksize)
        y3 = y.reshape(B, Lpad, C)
        for b, Lb in enumerate(lens):
            assert torch.count_nonzero(y3[b, Lb:]).item() == 0
            xs = x[b, :Lb].double().T[None]                                   # (1, C, Lb)
            ref = F.conv1d(xs, w.double()[:, None, :], bias.double(), padding=R, groups=C)[0].T
            err = rel_l2(y3[b, :Lb].cpu().double(), ref)
            assert err <= (1e-6 if dtype == torch.float32 else 4e-3), (Lpad, Lb, err)
            ys = torch.empty(Lb, C, dtype=dtype, device=dev)
            ops.dwconv(xd.reshape(B, Lpad, C)[b, :Lb].contiguous(), w.to(dev), bias.to(dev), ys, 1, Lb, ksize)
            assert torch.equal(y3[b, :Lb], ys), (Lpad, Lb)


# ---------------------------------------------------------------- u-head (+ tail)
def _uhead_ref(xs, W):
    """xs: (E, Lb) fp64; the u_head stack (model.py:58-65) and its mean over the sequence's own frames."""
    w0, b0, w1, b1, w3, b3, w4, b4 = (t.double() for t in W)
    E, U = w0.shape[0], w1.shape[0]
    z = F.conv1d(xs[None], w0[:, None, :], b0, padding=1, groups=E)
    z = F.silu(F.conv1d(z, w1[:, :, None], b1))
    z = F.conv1d(z, w3[:, None, :], b3, padding=1, groups=U)
    z = F.silu(F.conv1d(z, w4[:, :, None], b4))
    return z[0].sum(-1)


def test_uhead_varlen(dev):
    gen = torch.Generator().manual_seed(5)
    E, U = 6, 32
    W = [torch.randn(E, 3, generator=gen) * 0.5, torch.randn(E, generator=gen) * 0.1, torch.randn(U, E, generator=gen) * 0.4,
         torch.randn(U, generator=gen) * 0.1, torch.randn(U, 3, generator=gen) * 0.5, torch.randn(U, generator=gen) * 0.1,
         torch.randn(U, U, generator=gen) * 0.2, torch.randn(U, generator=gen) * 0.1]
    Wd = [t.to(dev) for t in W]
    w_out, b_out, u_scale = torch.randn(U, generator=gen) * 0.3, torch.randn(1, generator=gen) * 0.1, 1.7
    for Lpad in (70, 211):
        lens = _lens_for(Lpad)
        B = len(lens)
        xt = torch.randn(B, E, Lpad, generator=gen)
        for b, Lb in enumerate(lens):
            xt[b, :, Lb:] = NAN
        lens_dev = torch.tensor(lens, dtype=torch.int32, device=dev)
        fsum = torch.zeros(B, U, device=dev)
        ops.uhead_fwd_varlen(xt.to(dev), Wd, fsum, lens_dev, U)
        mod = torch.randn(B, 2 * U, generator=gen) * 0.2
        u = torch.full((B,), NAN, device=dev)
        ops.uhead_tail_varlen(fsum, mod.to(dev), w_out.to(dev), b_out.to(dev), u, lens_dev, Lpad, u_scale)
        for b, Lb in enumerate(lens):
            ref = _uhead_ref(xt[b, :, :Lb].double(), W)
            assert rel_l2(fsum[b].cpu(), ref) <= 1e-5, (Lpad, Lb)
            f = ref / Lb
            y = (w_out.double() * (f * (1 + mod[b, :U].double()) + mod[b, U:].double())).sum() + b_out.double()
            uref = u_scale * F.softplus(y)
            assert abs(float(u[b]) - float(uref)) <= 1e-5 * abs(float(uref)) + 1e-6, (Lpad, Lb, float(u[b]), float(uref))
            # the sequence alone through the non-varlen kernels (same windows, same sums: at most the last bits of the atomics' order)
            fs = torch.zeros(1, U, device=dev)
            ops.uhead_fwd(xt[b:b + 1, :, :Lb].contiguous().to(dev), Wd, fs, U)
            assert rel_l2(fsum[b:b + 1].cpu(), fs.cpu()) <= 1e-6, (Lpad, Lb)


# ---------------------------------------------------------------- sampler: grouped eta, varlen step
def test_sampler_eta_groups_and_step_varlen(dev):
    gen = torch.Generator().manual_seed(9)
    offs = [0, 2, 6, 7, 77]                       # groups of 2, 4, 1 and 70 rows (more than one wave's worth)
    G, B, E, Lpad = len(offs) - 1, offs[-1], 6, 130
    c0, num_steps = 0.05, 8
    u = (torch.rand(B, generator=gen) * 2 + 0.1).to(dev)
    offs_dev = torch.tensor(offs, dtype=torch.int32, device=dev)
    eta = torch.full((G, 2), NAN, device=dev)
    ops.sampler_eta_groups(u, offs_dev, eta, c0, num_steps)
    for g in range(G):
        e1 = torch.full((2,), NAN, device=dev)
        ops.sampler_eta(u[offs[g]:offs[g + 1]].contiguous(), e1, c0, num_steps)
        assert torch.equal(eta[g].view(torch.int32), e1.view(torch.int32)), g
    # lengths: one per song, every row of a song the same
    glens = [1, 64, 65, Lpad]
    lens = [glens[g] for g in range(G) for _ in range(offs[g], offs[g + 1])]
    x = torch.randn(B, E, Lpad, generator=gen)
    v = torch.randn(B, E, Lpad, generator=gen)
    for b, Lb in enumerate(lens):
        x[b, :, Lb:] = NAN
        v[b, :, Lb:] = NAN
    xd, vd = x.clone().to(dev), v.to(dev)          # (clone: on the emulator .to() would alias x)
    ops.sampler_step_varlen(xd, u, vd, eta, torch.tensor(lens, dtype=torch.int32, device=dev), offs_dev)
    for g in range(G):
        r0, r1, Lg = offs[g], offs[g + 1], glens[g]
        assert torch.count_nonzero(xd[r0:r1, :, Lg:]).item() == 0, g
        xs = x[r0:r1, :, :Lg].contiguous().to(dev)
        ops.sampler_step(xs, u[r0:r1].contiguous(), v[r0:r1, :, :Lg].contiguous().to(dev), eta[g].contiguous())
        assert torch.equal(xd[r0:r1, :, :Lg].view(torch.int32), xs.view(torch.int32)), g
