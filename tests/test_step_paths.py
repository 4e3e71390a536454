"""The kernels that close every training step and every sampler step — optimizer, loss, sampler, the per-sample linears, weight packing, the
element-wise boundary kernels, the style forward and the deterministic accumulator — against fp64 restatements of their formulas evaluated
on the operands and scalars as the kernel receives them (fp32 / bf16 rounded, hyper-parameters rounded to fp32).

Dispatch table (osu_dreamer_amd/csrc/optim.hip, heads.hip, misc.hip, style.hip, det.hip).  The path functions below mirror the launchers'
grid rules; `test_step_dispatch_table_matches_sources` re-reads the constants from the sources (SQ_MAX_BLOCKS 2048, the 4096-block and
256-block grid caps, LS_KC 256, LS_NB 8, LS_NR 32, SC_FT 16, SC_BS 64, the 64-lane loops) and checks that the cases of this file reach
every row on each backend.  A cap that changes fails that test, which names the case to resize.

  row                         kernel                           reached by (smallest shape)
  sqnorm/one                  sqnorm_kernel, 1 block           n in {1, 3, 4, 1027}: block 0 also owns the n % 4 tail
  sqnorm/multi                last-arrival sum of the slots    n = 4 256 3 + 2 (3 blocks)
  sqnorm/cap                  SQ_MAX_BLOCKS blocks, stride     n = 2048 1024 + 5 (2049 -> 2048 blocks), 3 2048 1024 + 3 (three strides)
  adamw/{one,multi,cap}       adamw_ema_kernel                 n in {1, 255} / 257 / 4096 256 + 77 (4097 -> 4096 blocks)
  ema/{one,multi,cap}         ema_kernel                       the same n
  loss/{one,multi,cap}        make_xt / loss_grad kernels      E L = 6 / 300 / 65550 (257 -> 256 blocks in x)
  loss/lanes{1,2}             loss_finalize_kernel             B <= 64 / B = 67 (second pass of the 64-lane loop)
  eta/lanes{1,2,3}            sampler_eta{,_groups}_kernel     B in {1, 64} / 65 / 130
  step{,_varlen}/{one,multi,cap}  sampler_step{,_varlen}_kernel  the loss shapes
  ls_fwd/kc{1,2,3}            linear_small_kernel              K <= 256 / 257 / 513: 256-deep chunks, 32 x 8 output tiles (ragged at B 33, N 9)
  ls_dw, ls_dx/nr{1,2,3}      linear_small_{dw,dx}_kernel      32-row slices of N meeting in dx: N <= 32 / 41 / 96
  pack/{bf16,fp32}{,/t}, pack/split   pack_weight{,_split}_kernel
  frames, silu{,_bwd}/{one,cap}, scale, cast                 cl_to_frames / silu / scale_channels / cast_rows kernels; silu cap: n = 8 (4096 256) + 8
  style_cond, rms_rows        style_cond_kernel, rmsnorm_rows_kernel   H > 256: two blocks in x; M = 5: two blocks of four rows
  det/{small,cap}             det_flush_kernel                 count <= 4096 256 / 4096 256 + 77
  GPU-only rows: none — the emulator runs every cap shape in a few seconds.

Memory contract: every output sits inside a wider NaN-prefilled buffer (64 NaN either side, or a NaN halo of rows and columns), every
operand inside a NaN-poisoned one.  Afterwards everything outside the output is still NaN and nothing inside is.  Accumulated outputs
(sqnorm's out, dsq, sums, dW, db, an accumulating dx) are prefilled with known finite values and must come out as prefill + sum.  All
operands are 16-byte aligned.

Bounds.  Outputs defined as exact (copies, casts, packing, t = 0 / 1, padding, skipped steps) are compared bit for bit.  For everything else
the same restated formula is ALSO evaluated in plain fp32 torch on the CPU; its error against fp64, in the same metric and over the same
block, times 4, and never less than 8 fp32 eps (9.5e-7), is the kernel's bound (`held()`): a different but legitimate summation order and
the device's expf / cosf / rsqrtf differ from torch's by a small factor, a missing term or a wrong index by orders of magnitude.  Element
errors are relative to |reference|, or to the sum of the absolute values of the terms where a result cancels (`scale=`; the linears' tiles
in the cancelling family, and their ragged corner tiles of fewer than 8 elements in every family; db element by element).  Deterministic mode
adds 2^-41 per contribution (the fixed-point step, rounded to nearest).  One exception, with its reason: od_silu / od_silu_grad evaluate
exp(-x) as the device's exp2 of the fp32 product -x log2(e); that product's rounding alone is a relative error of |x| 2^-24 in the
exponential, which torch's expf does not have.  Where x < 0 (elsewhere exp(-x) is small beside 1) SiLU rows therefore get (8 + |x|) eps as their floor instead of 8 eps.

What catches what in adamw_ema_kernel (each deletion made once by hand in a scratch copy of optim.hip and run on the emulator; p is the
first buffer checked, so a case that fails fails on p):
  `* (1.f - lr * wd)` dropped      test_adamw p of every wd = 0.01 case (family small: 1e-4 of |p| against a bound of 1e-6; family unit:
                                   1e-4 |p| = 800 ulp(p)); the wd = 0 cases pass, as they must
  `/ bc1` dropped                  test_adamw p at steps 1, 2, 3 (the update is off by 1 / bc1 = 10, 5.3, 3.7); step 1000 has bc1 = 1
  `/ bc2_sqrt` dropped             test_adamw p at every step (sqrt(1 - b2^1000) = 0.795), all families but `eps`
  `+ eps` dropped                  test_adamw p of family `eps` (v = 0, g = 0: denom = eps exactly; without it p is Inf / NaN) and of family
                                   `span` (|g| down to 2^-60: sqrt(v) far under eps); nothing else sees 1e-8
  `* clip` dropped                 test_adamw p of the clip-active cases of every family (m and v start non-zero, so p is not scale-free in
                                   g; m and v are off by the factor too); test_adamw_nonfinite_norm at an Inf norm (clip 0)
  every one of the five            test_adamw_against_torch (three chained steps against torch.optim.AdamW + clip_grad_norm_ + lerp)
That last test also found the one defect of this file's kernels: od_adamw_ema formed the bias corrections as 1.f - powf(beta, step) in fp32.
At step 2 the power's half ulp is 1.5e-5 of bc2 = 2e-3 and 7e-6 of the update, 7 x the fp32 recipe's whole error; the host now forms them in
double, as torch does, and hands them over rounded to fp32.

Non-finite norm (status 0): the kernel's clip is `c < 1 ? c : 1` with c = max_norm / (sqrt(gnorm_sq) + 1e-6).  A NaN norm gives c = NaN and
clip 1: the step goes ahead unclipped, and only the elements whose own gradient is NaN become NaN.  torch's clip_grad_norm_ multiplies
every gradient by clamp(NaN, max = 1) = NaN: all parameters become NaN.  An Inf norm gives clip 0 in both: finite gradients become 0 (the
step is decay and momentum only), an Inf gradient becomes Inf 0 = NaN.  `test_adamw_nonfinite_norm` pins the kernel's side.

Measured worst errors (kernel error / its bound, worst block of the worst case of the row; emulator | MI355X):
  row              output        emulator: error / bound     MI355X: error / bound
  adamw/cap        ema           6.42e-07 / 2.57e-06         9.49e-07 / 2.57e-06
  adamw/cap        m             1.38e-07 / 9.54e-07         1.15e-07 / 9.54e-07
  adamw/cap        p             6.42e-07 / 2.57e-06         9.49e-07 / 2.57e-06
  adamw/cap        v             1.33e-07 / 9.54e-07         1.19e-07 / 9.54e-07
  adamw/multi      ema           1.43e-07 / 9.54e-07         1.74e-07 / 9.54e-07
  adamw/multi      m             1.37e-07 / 9.54e-07         1.58e-07 / 9.54e-07
  adamw/multi      nonfinite-ema 6.18e-08 / 9.54e-07         5.85e-08 / 9.54e-07
  adamw/multi      nonfinite-m   1.05e-07 / 9.54e-07         1.05e-07 / 9.54e-07
  adamw/multi      nonfinite-p   1.57e-07 / 9.54e-07         1.78e-07 / 9.54e-07
  adamw/multi      nonfinite-v   1.12e-07 / 9.54e-07         1.12e-07 / 9.54e-07
  adamw/multi      p             1.52e-07 / 9.54e-07         1.74e-07 / 9.54e-07
  adamw/multi      torch-ema     8.72e-08 / 9.54e-07         9.33e-08 / 9.54e-07
  adamw/multi      torch-m       1.20e-07 / 9.54e-07         9.64e-08 / 9.54e-07
  adamw/multi      torch-p       2.11e-07 / 1.00e-06         1.56e-07 / 1.00e-06
  adamw/multi      torch-v       2.03e-07 / 1.24e-06         2.03e-07 / 1.24e-06
  adamw/multi      v             1.10e-07 / 9.54e-07         1.10e-07 / 9.54e-07
  adamw/one        ema           1.40e-07 / 9.54e-07         1.40e-07 / 9.54e-07
  adamw/one        m             9.91e-08 / 9.54e-07         9.91e-08 / 9.54e-07
  adamw/one        p             1.79e-07 / 9.54e-07         1.79e-07 / 9.54e-07
  adamw/one        v             1.07e-07 / 9.54e-07         1.07e-07 / 9.54e-07
  ema/cap          ema           7.59e-08 / 9.54e-07         5.84e-08 / 9.54e-07
  ema/multi        ema           5.48e-08 / 9.54e-07         5.48e-08 / 9.54e-07
  ema/one          ema           5.54e-08 / 9.54e-07         5.54e-08 / 9.54e-07
  eta/lanes1       eta           7.89e-08 / 9.54e-07         7.89e-08 / 9.54e-07
  eta/lanes2       eta           1.32e-07 / 9.54e-07         1.32e-07 / 9.54e-07
  eta/lanes3       eta           9.60e-08 / 9.54e-07         9.60e-08 / 9.54e-07
  loss/cap         dsq           4.19e-07 / 9.54e-07         1.30e-07 / 9.54e-07
  loss/cap         dv            2.07e-07 / 9.54e-07         2.07e-07 / 9.54e-07
  loss/cap         sums          1.78e-07 / 9.54e-07         2.37e-07 / 9.54e-07
  loss/cap         xt            9.95e-08 / 9.54e-07         9.95e-08 / 9.54e-07
  loss/lanes1      du            8.67e-08 / 9.54e-07         8.67e-08 / 9.54e-07
  loss/lanes1      out           9.92e-08 / 9.54e-07         1.07e-07 / 9.54e-07
  loss/lanes2      du            1.42e-07 / 9.54e-07         1.42e-07 / 9.54e-07
  loss/lanes2      out           1.17e-07 / 9.54e-07         1.04e-07 / 9.54e-07
  loss/multi       dsq           1.38e-04 / 5.53e-04         1.38e-04 / 5.53e-04
  loss/multi       dv            2.55e-07 / 1.02e-06         2.58e-07 / 1.03e-06
  loss/multi       sums          1.59e-07 / 9.54e-07         1.49e-07 / 9.54e-07
  loss/multi       xt            9.52e-08 / 9.54e-07         9.52e-08 / 9.54e-07
  loss/one         dsq           5.13e-08 / 9.54e-07         5.13e-08 / 9.54e-07
  loss/one         dv            8.60e-08 / 9.54e-07         8.23e-08 / 9.54e-07
  loss/one         sums          1.00e-07 / 9.54e-07         7.90e-08 / 9.54e-07
  loss/one         xt            5.60e-08 / 9.54e-07         5.60e-08 / 9.54e-07
  ls_dw            dW            1.31e-07 / 9.54e-07         1.31e-07 / 9.54e-07
  ls_dw            db            1.85e-07 / 9.54e-07         1.96e-07 / 9.54e-07
  ls_dw            dpre          8.92e-08 / 9.79e-07         2.72e-06 / 7.87e-06
  ls_dx/nr1        dx            9.39e-08 / 9.54e-07         6.59e-08 / 9.54e-07
  ls_dx/nr2        dx            1.41e-07 / 9.54e-07         1.34e-07 / 9.54e-07
  ls_dx/nr3        dx            1.17e-07 / 9.54e-07         1.12e-07 / 9.54e-07
  ls_fwd/kc1       out           2.77e-07 / 1.16e-06         2.78e-07 / 9.54e-07
  ls_fwd/kc1       pre           2.37e-07 / 9.70e-07         2.78e-07 / 9.54e-07
  ls_fwd/kc2       out           5.03e-07 / 9.54e-07         4.58e-07 / 9.54e-07
  ls_fwd/kc2       pre           5.53e-07 / 9.54e-07         5.41e-07 / 1.07e-06
  ls_fwd/kc3       out           4.95e-07 / 9.91e-07         5.27e-07 / 9.54e-07
  ls_fwd/kc3       pre           5.15e-07 / 9.54e-07         5.59e-07 / 9.54e-07
  rms_rows         y             9.02e-08 / 9.54e-07         7.45e-08 / 9.54e-07
  silu/cap         silu-bf16     3.89e-03 / 3.89e-03         3.89e-03 / 3.89e-03
  silu/cap         silu-fp32     1.44e-07 / 9.57e-07         5.01e-07 / 1.63e-06
  silu/one         silu-bf16     1.68e-03 / 2.77e-03         1.68e-03 / 2.77e-03
  silu/one         silu-fp32     2.59e-08 / 9.54e-07         1.87e-06 / 1.15e-05
  silu_bwd/cap     silu_bwd-bf16 3.89e-03 / 3.89e-03         3.89e-03 / 3.89e-03
  silu_bwd/cap     silu_bwd-fp32 3.24e-07 / 9.54e-07         4.98e-07 / 9.74e-07
  silu_bwd/one     silu_bwd-bf16 2.27e-03 / 2.54e-03         2.27e-03 / 2.54e-03
  silu_bwd/one     silu_bwd-fp32 1.23e-08 / 9.54e-07         1.85e-06 / 1.17e-05
  sqnorm/cap       out           5.02e-08 / 9.54e-07         5.02e-08 / 9.54e-07
  sqnorm/multi     out           9.86e-08 / 9.54e-07         9.86e-08 / 9.54e-07
  sqnorm/one       out           5.76e-08 / 9.54e-07         5.76e-08 / 9.54e-07
  step/cap         x             1.15e-07 / 9.54e-07         7.33e-08 / 9.54e-07
  step/multi       x             1.16e-07 / 9.54e-07         9.44e-08 / 9.54e-07
  step/one         x             1.74e-08 / 9.54e-07         1.74e-08 / 9.54e-07
  step_varlen/cap  x             1.02e-07 / 9.54e-07         5.94e-08 / 9.54e-07
  step_varlen/multi x             8.73e-08 / 9.54e-07         8.61e-08 / 9.54e-07
  step_varlen/one  x             2.80e-08 / 9.54e-07         1.71e-08 / 9.54e-07
  style_cond       c             1.63e-07 / 9.54e-07         1.63e-07 / 9.54e-07
"""
import math
import os
import re
from dataclasses import dataclass

import pytest
import torch

from osu_dreamer_amd import _lib, det, ops
from osu_dreamer_amd._lib import OD_ACT_NONE, OD_ACT_SILU, HipKernelError
from kernel_backend import REPO, Fenced, Flat, bits, det_run, dev, tile_errors  # noqa: F401

CSRC = os.path.join(REPO, "osu_dreamer_amd", "csrc")
NAN, INF = float("nan"), float("inf")
EPS32 = 2.0 ** -23
FLOOR = 8 * EPS32
SQ_MAX_BLOCKS, CAP_1D, CAP_X, LANES = 2048, 4096, 256, 64
LS_KC, LS_NB, LS_NR, SC_FT, SC_BS = 256, 8, 32, 16, 64
TINY = 2.0 ** -126 / FLOOR                  # added to a scale: an error under fp32's smallest normal (where exp(-x) has overflowed) always passes
FIX = 2.0 ** -41                            # half a step of the deterministic shadow


def cdiv(a, b):
    return (a + b - 1) // b


def f32(x):
    return float(torch.tensor(x, dtype=torch.float32))


def gen(seed):
    return torch.Generator().manual_seed(seed)


# ---------------------------------------------------------------- path functions (the table above)
def sq_path(n):
    b = cdiv(n // 4, 256)
    return "sqnorm/one" if b <= 1 else ("sqnorm/cap" if b > SQ_MAX_BLOCKS else "sqnorm/multi")


def flat_path(kind, n, per=1):
    b = cdiv(n // per, 256)
    return f"{kind}/one" if b <= 1 else (f"{kind}/cap" if b > CAP_1D else f"{kind}/multi")


def x_path(kind, E, L):
    b = cdiv(E * L, 256)
    return f"{kind}/one" if b <= 1 else (f"{kind}/cap" if b > CAP_X else f"{kind}/multi")


def lane_path(kind, B):
    return f"{kind}/lanes{cdiv(B, LANES)}"


ROWS = (["sqnorm/one", "sqnorm/multi", "sqnorm/cap"] + [f"{k}/{s}" for k in ("adamw", "ema", "loss", "step", "step_varlen") for s in ("one", "multi", "cap")]
        + ["loss/lanes1", "loss/lanes2", "eta/lanes1", "eta/lanes2", "eta/lanes3"] + [f"ls_fwd/kc{i}" for i in (1, 2, 3)] + ["ls_dw"]
        + [f"ls_dx/nr{i}" for i in (1, 2, 3)] + ["pack/bf16", "pack/bf16/t", "pack/fp32", "pack/fp32/t", "pack/split", "frames", "silu/one", "silu/cap",
                                                 "silu_bwd/one", "silu_bwd/cap", "scale", "cast", "style_cond", "rms_rows", "det/small", "det/cap"])
GPU_ONLY_ROWS = []
REACHED = set()                             # filled at import by the case tables below


# ---------------------------------------------------------------- the bound
def rel(a, ref, scale=None):
    """|a - ref| / scale per element in fp64 on the CPU (scale: |ref| unless given).  0 where the two agree exactly (Inf and NaN included),
    Inf where they do not and the scale is 0, or where exactly one of them is NaN."""
    a, ref = a.detach().double().cpu(), ref.detach().double().cpu()
    den = ref.abs() if scale is None else scale.detach().double().cpu()
    same = (a == ref) | (torch.isnan(a) & torch.isnan(ref))
    e = torch.where(same, torch.zeros_like(ref), (a - ref).abs() / den)
    return torch.nan_to_num(e, nan=INF, posinf=INF)


def held(case, row, what, device, out, ref, ref32, scale=None, extra=0.0, group=None, floor=FLOOR):
    """The kernel's error against fp64 is within 4 x the plain fp32 evaluation's (and `floor`), block by block.  `group` maps the element
    errors to per-block maxima (default: one block); `extra` is added to the bound (the deterministic shadow's step)."""
    ek, e32 = rel(out, ref, scale), rel(ref32, ref, scale)
    fl = floor if isinstance(floor, float) else floor.double().cpu()
    if group is not None:
        ek, e32 = group(ek), group(e32)
        fl = fl if isinstance(fl, float) else group(fl)
    elif ek.numel():
        ek, e32 = ek.max().reshape(1), e32.max().reshape(1)
        fl = fl if isinstance(fl, float) else fl.max().reshape(1)
    bound = torch.maximum(4 * e32, torch.as_tensor(fl, dtype=torch.float64).expand_as(e32)) + extra
    ratio = ek / bound
    if ratio.numel():
        w = int(ratio.flatten().argmax())
        print(f"MEASURED {row} {what} {'hip' if device.type == 'cuda' else 'emu'} {float(ek.flatten()[w]):.3e} {float(bound.flatten()[w]):.3e} {case}")
        assert float(ratio.flatten()[w]) <= 1.0, (f"{case} {what}: block {w} error {float(ek.flatten()[w]):.3e} > bound {float(bound.flatten()[w]):.3e} "
                                                   f"(fp32 torch {float(e32.flatten()[w]):.3e})")


def half_ulp_bf16(ref):
    """Half a bf16 ulp of every element of the fp64 tensor `ref`: 2^(floor(log2 |ref|) - 8), the normal range's smallest below it."""
    _, e = torch.frexp(torch.nan_to_num(ref.abs(), nan=0.0, posinf=0.0))             # |ref| = m 2^e, m in [0.5, 1)
    return torch.ldexp(torch.ones_like(ref), e.clamp_min(-125) - 9)


def same_bits(case, what, a, b):
    assert a.shape == b.shape and torch.equal(bits(a.contiguous()).cpu(), bits(b.contiguous()).cpu()), f"{case}: {what} differs bit for bit"


def poisoned(t, device, dtype=None):
    """`t` as the kernel's operand: inside a NaN buffer (integers: a buffer of -2^30), 64 elements either side, on `device`."""
    t = t if dtype is None else t.to(dtype)
    if t.is_floating_point():
        return Flat(tuple(t.shape), device, fill=t.to(device), dtype=t.dtype).v
    buf = torch.full((t.numel() + 128,), -2 ** 30, dtype=t.dtype, device=device)
    buf[64:64 + t.numel()] = t.flatten().to(device)
    return buf[64:64 + t.numel()].view(t.shape)


def raises(code, fn):
    with pytest.raises(HipKernelError, match=f"code {code}:"):
        fn()


ERR_ARG, ERR_ALIGN, ERR_UNSUPPORTED = -1, -2, -3


# ================================================================ optimizer
SQ_NS = (1, 3, 4, 1027, 4 * 256 * 3 + 2, 2048 * 1024 + 5, 3 * 2048 * 1024 + 3)
SQ_FAMS = ("random", "big", "tail", "last_block", "zero_slab")
REACHED |= {sq_path(n) for n in SQ_NS}


def sq_input(fam, n, g):
    x = torch.randn(n, generator=g)
    if fam == "big":
        x *= 1e-3
        x[int(torch.randint(0, n, (1,), generator=g))] = 1e18
    elif fam == "tail":                      # the n % 4 elements block 0 adds on its own (n % 4 = 0: the last element)
        keep = max(n % 4, 1)
        x[:n - keep] = 0
    elif fam == "last_block":                # the f32x4 range of the last block's first stride
        blocks = min(max(cdiv(n // 4, 256), 1), SQ_MAX_BLOCKS)
        x[:4 * 256 * (blocks - 1)] = 0
        x[min(4 * 256 * blocks, n // 4 * 4):] = 0
        if n < 4:
            x[:] = 0
    elif fam == "zero_slab":
        x[n // 4:n // 2 + 1] = 0
    return x


@pytest.mark.parametrize("fam", SQ_FAMS)
@pytest.mark.parametrize("n", SQ_NS)
def test_sqnorm(dev, n, fam):
    case = f"sqnorm-{fam}-{n}"
    x = sq_input(fam, n, gen(n % 1000 + len(fam)))
    xd = poisoned(x, dev)
    ref = 2.0 + x.double().pow(2).sum()
    ref32 = (torch.tensor(2.0) + (x * x).sum()).reshape(1)
    outs = []
    for status in (None, 0, None):
        out = Flat((1,), dev, fill=torch.tensor([2.0]))
        st = None if status is None else poisoned(torch.tensor([status], dtype=torch.int32), dev)
        ops.sqnorm(xd, out.v, 0 if st is None else st.data_ptr())
        out.check(case, "out")
        outs.append(out.v.clone())
    held(case, sq_path(n), "out", dev, outs[0], ref.reshape(1), ref32)          # all terms are >= 0: relative to the sum itself
    same_bits(case, "out of a second launch on the same input (the order-free sum)", outs[0], outs[2])
    same_bits(case, "out with status = 0", outs[0], outs[1])
    out = Flat((1,), dev, fill=torch.tensor([2.0]))
    st = poisoned(torch.tensor([7], dtype=torch.int32), dev)
    ops.sqnorm(xd, out.v, st.data_ptr())
    assert bool(torch.isnan(out.v).all()), f"{case}: a non-zero status word must poison the norm"
    assert int(st[0]) == 7
    out2 = Flat((1,), dev, fill=torch.tensor([2.0]))                           # and the poisoned launch left the arrival counter re-armed
    ops.sqnorm(xd, out2.v)
    same_bits(case, "out after a poisoned launch", outs[0], out2.v)


LR, B1, B2, AEPS, WD, DECAY = (f32(v) for v in (1e-2, 0.9, 0.999, 1e-8, 0.01, 0.99))
ADAM_NS = (1, 255, 257, 4096 * 256 + 77)
REACHED |= {flat_path(k, n) for n in ADAM_NS for k in ("adamw", "ema")}


def clip_of(gn_sq, max_norm, dt):
    """The kernel's clip factor from the fp32 norm word, in `dt`."""
    if gn_sq is None or not max_norm > 0:
        return torch.tensor(1.0, dtype=dt)
    c = torch.tensor(max_norm, dtype=dt) / (gn_sq.to(dt).sqrt() + torch.tensor(f32(1e-6), dtype=dt))
    return c if bool(c < 1) else torch.tensor(1.0, dtype=dt)


def adam_formula(p, g, m, v, e, step, mode, clip, wd, dt):
    """One AdamW + EMA step as the kernel states it, in `dt`.  Returns the new (p, m, v, ema) and the |terms| scale of each."""
    T = lambda s: torch.tensor(s, dtype=dt)      # noqa: E731
    p, g, m, v = p.to(dt), g.to(dt), m.to(dt), v.to(dt)
    one = T(1.0)
    bc1, bc2s = T(f32(1.0 - B1 ** step)), T(f32(math.sqrt(1.0 - B2 ** step)))      # formed by the host in double, handed over as fp32
    gi = g * clip.to(dt)
    pd = p * (one - T(LR) * T(wd))
    mi = T(B1) * m + (one - T(B1)) * gi
    vi = T(B2) * v + (one - T(B2)) * gi * gi
    upd = (T(LR) / bc1) * (mi / (vi.sqrt() / bc2s + T(AEPS)))
    pn = pd - upd
    out = [pn, mi, vi]
    sc = [pd.abs() + upd.abs(), (T(B1) * m).abs() + ((one - T(B1)) * gi).abs(), vi.abs()]
    if mode == 1:
        out.append(pn.clone()); sc.append(sc[0])
    elif mode == 2:
        e = e.to(dt)
        out.append(e + (one - T(DECAY)) * (pn - e)); sc.append(e.abs() + (one - T(DECAY)) * (pn.abs() + e.abs()))
    return out, sc


@dataclass(frozen=True)
class AC:
    n: int
    step: int
    mode: int
    clip: str            # active / inactive / zero (max_norm = 0) / null (gnorm_sq = NULL)
    wd: float
    fam: str             # small (|p| <= lr) / unit (|p| ~ 1) / eps (v = 0, g = 0) / span (|g| from 2^-60 to 2^20)

    @property
    def id(self):
        return f"adamw-{self.fam}-n{self.n}-s{self.step}-ema{self.mode}-clip_{self.clip}-wd{self.wd:g}"


def _adam_cases():
    out, i = [], 0
    clips, fams = ("active", "inactive", "zero", "null"), ("small", "unit")
    for n in ADAM_NS[:3]:
        for step in (1, 2, 3, 1000):
            for mode in (0, 1, 2):
                out.append(AC(n, step, mode, clips[i % 4], WD if (i // 4) % 2 == 0 else 0.0, fams[(i // 2) % 2]))
                i += 1
    for fam in ("small", "unit"):            # every clip kind and both decays on both families at one size
        for clip in clips:
            for wd in (0.0, WD):
                out.append(AC(257, 2, 2, clip, wd, fam))
    out += [AC(n, s, 2, "active", WD, f) for f in ("eps", "span") for n, s in ((255, 1), (257, 1000))]
    out += [AC(ADAM_NS[3], 3, 2, "active", WD, "small"), AC(ADAM_NS[3], 1, 1, "null", 0.0, "unit"), AC(ADAM_NS[3], 1000, 0, "inactive", WD, "span")]
    return list(dict.fromkeys(out))


ADAM_CASES = _adam_cases()


def adam_inputs(c, g):
    n = c.n
    p = (LR * (2 * torch.rand(n, generator=g) - 1)) if c.fam in ("small", "eps", "span") else torch.randn(n, generator=g)
    gr = torch.randn(n, generator=g)
    m = 0.3 * torch.randn(n, generator=g)
    v = 0.5 * torch.rand(n, generator=g) + 1e-3
    if c.fam == "eps":
        gr, v, m = torch.zeros(n), torch.zeros(n), 1e-8 * torch.randn(n, generator=g)
    elif c.fam == "span":
        gr = gr.sign() * 2.0 ** torch.randint(-60, 21, (n,), generator=g).float()
        m, v = gr * (2 * torch.rand(n, generator=g) - 1), gr * gr * (0.5 + 1.5 * torch.rand(n, generator=g))
    e = p + 0.1 * LR * torch.randn(n, generator=g)
    return p, gr, m, v, e


def run_adam(device, c, p, gr, m, v, e, gn, max_norm, status=None):
    bufs = [Flat((c.n,), device, fill=t) for t in (p, m, v)] + ([Flat((c.n,), device, fill=e)] if c.mode else [])
    ops.adamw_ema(bufs[0].v, poisoned(gr, device), bufs[1].v, bufs[2].v, bufs[3].v if c.mode else None, LR, B1, B2, AEPS, c.wd, c.step, DECAY,
                  c.mode, None if gn is None else poisoned(gn, device), max_norm, 0 if status is None else status.data_ptr())
    return bufs


@pytest.mark.parametrize("c", ADAM_CASES, ids=lambda c: c.id)
def test_adamw(dev, c):
    p, gr, m, v, e = adam_inputs(c, gen(c.n % 997 + c.step + 7 * c.mode))
    norm = float(gr.double().pow(2).sum().sqrt())
    gn = None if c.clip == "null" else gr.double().pow(2).sum().float().reshape(1)
    max_norm = {"active": f32(0.5 * norm), "inactive": f32(2 * norm + 1), "zero": 0.0, "null": 1.0}[c.clip]
    bufs = run_adam(dev, c, p, gr, m, v, e, gn, max_norm)
    gsq = None if gn is None else gn[0]
    ref, sc = adam_formula(p, gr, m, v, e, c.step, c.mode, clip_of(gsq, max_norm, torch.float64), c.wd, torch.float64)
    r32, _ = adam_formula(p, gr, m, v, e, c.step, c.mode, clip_of(gsq, max_norm, torch.float32), c.wd, torch.float32)
    assert (float(clip_of(gsq, max_norm, torch.float64)) < 1) == (c.clip == "active" and c.fam != "eps")
    for b, name, r, r3, s in zip(bufs, ("p", "m", "v", "ema"), ref, r32, sc):
        b.check(c.id, name)
        held(c.id, flat_path("adamw", c.n), name, dev, b.v, r, r3, scale=s)
    if c.clip == "inactive":                 # a norm under max_norm is no clip at all: the bits of max_norm = 0
        for b, b0, name in zip(bufs, run_adam(dev, c, p, gr, m, v, e, gn, 0.0), ("p", "m", "v", "ema")):
            same_bits(c.id, f"{name} against max_norm = 0", b.v, b0.v)
    if c.step == 2:                          # a failed launch's status word: the step is skipped, every buffer keeps its bits; 0 is no status
        st = poisoned(torch.tensor([3], dtype=torch.int32), dev)
        for b, t, name in zip(run_adam(dev, c, p, gr, m, v, e, gn, max_norm, st), (p, m, v, e), ("p", "m", "v", "ema")):
            same_bits(c.id, f"{name} of a skipped step", b.v, t)
            b.check(c.id, name)
        st = poisoned(torch.tensor([0], dtype=torch.int32), dev)
        for b, b0, name in zip(bufs, run_adam(dev, c, p, gr, m, v, e, gn, max_norm, st), ("p", "m", "v", "ema")):
            same_bits(c.id, f"{name} with status = 0", b.v, b0.v)


def test_adamw_against_torch(dev):
    """Three chained steps (od_sqnorm -> od_adamw_ema) against torch.optim.AdamW + clip_grad_norm_ + the EMA lerp in fp64; the bound is the
    same recipe run in fp32.  |p| <= lr, so the updates are not below p's ulp; every step is clipped."""
    n, max_norm = 257, 1.0
    g = gen(5)
    p0 = LR * (2 * torch.rand(n, generator=g) - 1)
    grads = [3 * torch.randn(n, generator=g) for _ in range(3)]

    def recipe(dt):
        P = torch.nn.Parameter(p0.to(dt).clone())
        opt = torch.optim.AdamW([P], lr=LR, betas=(B1, B2), eps=AEPS, weight_decay=WD)
        ema, moved, mterms = None, p0.double().abs(), torch.zeros(n, dtype=torch.float64)
        for gr in grads:
            before = P.detach().double().clone()
            P.grad = gr.to(dt).clone()
            torch.nn.utils.clip_grad_norm_([P], max_norm)
            opt.step()
            moved = moved + (P.detach().double() - before).abs()
            mterms = B1 * mterms + (1 - B1) * P.grad.detach().double().abs()          # |terms| of exp_avg (the gradient as clipped)
            ema = P.detach().clone() if ema is None else ema.lerp(P.detach(), torch.tensor(1 - DECAY, dtype=dt))
        st = opt.state[P]
        return (P.detach(), st["exp_avg"], st["exp_avg_sq"], ema), moved, mterms

    ref, moved, mterms = recipe(torch.float64)
    r32, _, _ = recipe(torch.float32)
    bufs = [Flat((n,), dev, fill=t) for t in (p0, torch.zeros(n), torch.zeros(n), torch.zeros(n))]
    for s, gr in enumerate(grads, 1):
        gn = Flat((1,), dev, fill=torch.zeros(1))
        gd = poisoned(gr, dev)
        ops.sqnorm(gd, gn.v)
        ops.adamw_ema(bufs[0].v, gd, bufs[1].v, bufs[2].v, bufs[3].v, LR, B1, B2, AEPS, WD, s, DECAY, 1 if s == 1 else 2, gn.v, max_norm)
    for b, name, r, r3, sc in zip(bufs, ("p", "m", "v", "ema"), ref, r32, (moved, mterms, None, moved)):
        b.check("adamw-torch", name)
        held("adamw-torch", "adamw/multi", f"torch-{name}", dev, b.v, r, r3, scale=sc)


@pytest.mark.parametrize("norm", (NAN, INF))
def test_adamw_nonfinite_norm(dev, norm):
    """Pinned, not endorsed: a NaN norm word is no clip (clip 1), an Inf one is clip 0 (see the module docstring for clip_grad_norm_)."""
    c = AC(257, 2, 2, "active", WD, "small")
    p, gr, m, v, e = adam_inputs(c, gen(11))
    gr[5] = norm
    bufs = run_adam(dev, c, p, gr, m, v, e, torch.tensor([norm]), 1.0)
    clip = torch.tensor(1.0 if math.isnan(norm) else 0.0)
    ref, sc = adam_formula(p, gr, m, v, e, c.step, c.mode, clip.double(), c.wd, torch.float64)
    r32, _ = adam_formula(p, gr, m, v, e, c.step, c.mode, clip, c.wd, torch.float32)
    for b, name, r, r3, s in zip(bufs, ("p", "m", "v", "ema"), ref, r32, sc):
        assert bool(torch.isnan(b.buf[:64]).all() & torch.isnan(b.buf[64 + b.n:]).all()), f"{name}: written outside the buffer"
        assert bool(torch.isnan(b.v[5])) and int(torch.isnan(b.v).sum()) == 1, f"{name}: only the element with the non-finite gradient is NaN"
        held(f"adamw-norm-{norm}", "adamw/multi", f"nonfinite-{name}", dev, b.v, r, r3, scale=s)


@pytest.mark.parametrize("mode", (1, 2))
@pytest.mark.parametrize("n", ADAM_NS)
def test_ema_update(dev, n, mode):
    g = gen(n % 991 + mode)
    p = torch.randn(n, generator=g)
    e = p + 0.01 * torch.randn(n, generator=g)
    eb = Flat((n,), dev, fill=e)
    pd = poisoned(p, dev)
    ops.ema_update(eb.v, pd, DECAY, mode)
    eb.check(f"ema-{n}-{mode}", "ema")
    same_bits(f"ema-{n}-{mode}", "p (read only)", pd, p)
    if mode == 1:
        same_bits(f"ema-{n}", "ema after the first update (a copy)", eb.v, p)
        return
    ref = e.double() + (1.0 - torch.tensor(DECAY, dtype=torch.float64)) * (p.double() - e.double())
    r32 = e + (1.0 - torch.tensor(DECAY)) * (p - e)
    held(f"ema-{n}", flat_path("ema", n), "ema", dev, eb.v, ref, r32, scale=e.abs() + (1 - DECAY) * (p.abs() + e.abs()))


def test_optimizer_argument_checks(dev):
    t = [poisoned(torch.ones(8), dev) for _ in range(5)]
    call = lambda n, step, mode, ema: _lib.lib().od_adamw_ema(t[0].data_ptr(), t[1].data_ptr(), t[2].data_ptr(), t[3].data_ptr(), ema, n, LR, B1,   # noqa: E731
                                                              B2, AEPS, WD, step, DECAY, mode, None, 0.0, None, 0)
    raises(ERR_ARG, lambda: call(8, 0, 0, None))
    raises(ERR_ARG, lambda: call(8, -1, 2, t[4].data_ptr()))
    raises(ERR_ARG, lambda: call(0, 1, 0, None))
    raises(ERR_ARG, lambda: call(-8, 1, 0, None))
    raises(ERR_ARG, lambda: call(8, 1, 1, None))
    raises(ERR_ARG, lambda: call(8, 1, 2, None))
    for mode in (0, 3):
        raises(ERR_ARG, lambda: ops.ema_update(t[0], t[1], DECAY, mode))
    raises(ERR_ARG, lambda: _lib.lib().od_ema_update(t[0].data_ptr(), t[1].data_ptr(), 0, DECAY, 1, 0))
    for x in t:
        assert bool((x == 1).all()), "a refused call must not write"


# ================================================================ loss and sampler
C0 = f32(0.01)
E = 6
LOSS_SHAPES = ((3, 50), (1, 1), (67, 43), (2, 10925))
TVALS = (0.0, 0.25, 0.5, 0.75, 1.0)
LOSS_FAMS = ("random", "close", "v_target", "u_hit", "batch_distinct")
WEIGHTS = ((1.0, 30.0), (0.0, 1.0), (1.0, 0.0))
REACHED |= {x_path(k, E, L) for _, L in LOSS_SHAPES for k in ("loss", "step", "step_varlen")} | {lane_path("loss", B) for B, _ in LOSS_SHAPES}


def lerp_formula(x0, x1, t):
    """torch.lerp's two branches, as make_xt_kernel states them; the |terms| scale of xt; dsq's terms."""
    w = t[:, None, None]
    d = x1 - x0
    xt = torch.where(w < 0.5, x0 + w * d, x1 - d * (1 - w))
    sc = torch.where(w < 0.5, x0.abs() + (w * d).abs(), x1.abs() + (d * (1 - w)).abs())
    return xt, sc


def loss_inputs(fam, B, L, shift, g):
    x0, x1 = torch.randn(B, E, L, generator=g), torch.randn(B, E, L, generator=g)
    t = torch.tensor([TVALS[(b + shift) % 5] for b in range(B)])
    if fam == "close":
        x0 = x1 + 1e-4 * torch.randn(B, E, L, generator=g)
    if fam == "batch_distinct":
        s = (10.0 ** (torch.arange(B) % 3).float())[:, None, None]
        x0, x1 = x0 * s, x1 * s
    return x0, x1, t


def loss_uv(fam, xt, x1, dsq, g):
    """u (B) and v (B, E, L) of the family, from the operands od_loss_grad receives."""
    B = xt.shape[0]
    ut = (dsq + C0).sqrt()
    tgt = (xt - x1) / ut[:, None, None]
    u = ut * (0.5 + 1.5 * torch.rand(B, generator=g))
    v = torch.randn(xt.shape, generator=g)
    if fam == "v_target":                    # s2 cancels
        v = tgt * (1 + 1e-4 * torch.randn(xt.shape, generator=g))
    elif fam == "u_hit":                     # xt - u v = x1: s1 and dS1/du cancel
        v, u = 0.7 * tgt, ut / 0.7
    elif fam == "batch_distinct":
        v = v * (10.0 ** (torch.arange(B) % 3).float())[:, None, None]
    return u, v


def loss_grad_formula(xt, x1, u, v, dsq, sums0, osl_w, del_w, dt):
    """loss_grad_kernel restated in `dt`: dv, sums (prefill + terms), and their |terms| scales."""
    B, _, L = xt.shape
    xt, x1, u, v, dsq = (t.to(dt) for t in (xt, x1, u, v, dsq))
    T = lambda s: torch.tensor(s, dtype=dt)      # noqa: E731
    ub = u[:, None, None]
    den = dsq + T(C0)
    ut = den.sqrt()[:, None, None]
    k1, k2, invL2 = (T(osl_w) / (T(float(B)) * den))[:, None, None], T(del_w) / T(float(B)), T(2.0) / T(float(L))
    r1 = xt - ub * v - x1
    tg = (xt - x1) / ut
    r2 = v - tg
    dv = k1 * invL2 * r1 * (-ub) + k2 * invL2 * r2
    a1 = xt.abs() + (ub * v).abs() + x1.abs()
    a2 = v.abs() + tg.abs()
    dv_sc = k1 * invL2 * a1 * ub.abs() + k2 * invL2 * (v.abs() + (xt.abs() + x1.abs()) / ut)
    sums = torch.stack([(r1 * r1).sum((1, 2)) / L, (r2 * r2).sum((1, 2)) / L, (r1 * -v).sum((1, 2)) * invL2], 1)
    s_sc = torch.stack([(a1 * a1).sum((1, 2)) / L, (a2 * a2).sum((1, 2)) / L, (a1 * v.abs()).sum((1, 2)) * invL2], 1)
    return dv, dv_sc, sums0.to(dt) + sums, sums0.abs().to(dt) + s_sc


def finalize_formula(sums, dsq, u, osl_w, del_w, dt):
    sums, dsq, u = sums.to(dt), dsq.to(dt), u.to(dt)
    T = lambda s: torch.tensor(s, dtype=dt)      # noqa: E731
    B = u.shape[0]
    den = dsq + T(C0)
    ut = den.sqrt()
    osl, dele, mape = (sums[:, 0] / den).sum() / B, sums[:, 1].sum() / B, ((u - ut) / ut).abs().sum() / B
    out = torch.stack([T(osl_w) * osl + T(del_w) * dele, osl, dele, mape])
    a_osl, a_del = (sums[:, 0] / den).abs().sum() / B, sums[:, 1].abs().sum() / B
    sc = torch.stack([T(osl_w) * a_osl + T(del_w) * a_del, a_osl, a_del, ((u.abs() + ut) / ut).sum() / B])
    return out, sc, T(osl_w) / (T(float(B)) * den) * sums[:, 2]


def frames64(e):
    """Element errors (B, E, L) -> worst per (batch row, 64-frame block)."""
    B, _, L = e.shape
    nb = cdiv(L, 64)
    return torch.nn.functional.pad(e, (0, nb * 64 - L)).reshape(B, E, nb, 64).amax((1, 3))


@dataclass(frozen=True)
class LC:
    B: int
    L: int
    fam: str = "random"
    w: int = 0           # index into WEIGHTS
    shift: int = 0       # t[b] = TVALS[(b + shift) % 5]
    det: bool = False

    @property
    def id(self):
        return f"loss-{self.fam}-w{self.w}-t{self.shift}{'-det' if self.det else ''}-{self.B}x{self.L}"


LOSS_CASES = ([LC(B, L, w=i % 3, shift=i) for i, (B, L) in enumerate(LOSS_SHAPES)] + [LC(1, 1, shift=s) for s in (0, 1, 3, 4)] + [LC(2, 10925, shift=4)]
              + [LC(B, L, f, w) for B, L in ((3, 50), (67, 43)) for f in LOSS_FAMS[1:] for w in (0, 1, 2)]
              + [LC(3, 50, "random", w) for w in (1, 2)] + [LC(B, L, f, 0, 1, True) for B, L in ((67, 43), (2, 10925)) for f in ("random", "v_target")])


@pytest.mark.parametrize("c", LOSS_CASES, ids=lambda c: c.id)
def test_loss(dev, c):
    """od_make_xt -> od_loss_grad -> od_loss_finalize, each against its formula on the operands it actually received (the kernel before it
    wrote them), and the written-out loss's fp64 autograd against those formulas."""
    B, L = c.B, c.L
    g = gen(B * 131 + L + len(c.fam))
    osl_w, del_w = (f32(w) for w in WEIGHTS[c.w])
    x0, x1, t = loss_inputs(c.fam, B, L, c.shift, g)
    x0d, x1d, td = (poisoned(a, dev) for a in (x0, x1, t))
    # dsq's prefill is of its contribution's size: in `close` about 1e-8, so den = dsq + c0 is c0 to 1e-6 (the regime the family is for)
    dsq0, sums0 = (1e-8 if c.fam == "close" else 0.25) * torch.rand(B, generator=g), torch.randn(B, 3, generator=g) * 0.5
    nblk = min(cdiv(E * L, 256), CAP_X)
    runs = []
    for _ in range(2 if c.det else 1):
        xt, dsq = Flat((B, E, L), dev), Flat((B,), dev, fill=dsq0)
        det_run(dev, c.det, [dsq.v], lambda: ops.make_xt(x0d, x1d, td, xt.v, dsq.v))
        xt.check(c.id, "xt"), dsq.check(c.id, "dsq")
        u, v = loss_uv(c.fam, xt.v.cpu(), x1, dsq.v.cpu(), gen(B + 3))
        ud, vd = poisoned(u, dev), poisoned(v, dev)
        dv, sums = Flat((B, E, L), dev), Flat((B, 3), dev, fill=sums0)
        det_run(dev, c.det, [sums.v], lambda: ops.loss_grad(xt.v, x1d, ud, vd, dsq.v, dv.v, sums.v, C0, osl_w, del_w))
        dv.check(c.id, "dv"), sums.check(c.id, "sums")
        out, du = Flat((4,), dev), Flat((B,), dev)
        ops.loss_finalize(sums.v, dsq.v, ud, out.v, du.v, C0, osl_w, del_w)
        out.check(c.id, "out"), du.check(c.id, "du")
        runs.append([a.v.clone() for a in (xt, dsq, dv, sums, out, du)])
    if c.det:
        for a, b, name in zip(runs[0], runs[1], ("xt", "dsq", "dv", "sums", "out", "du")):
            same_bits(c.id, f"{name} of two deterministic runs", a, b)
    xt_k, dsq_k, dv_k, sums_k, out_k, du_k = (a.cpu() for a in runs[0])
    fix = nblk * FIX if c.det else 0.0
    # make_xt
    xr, xs = lerp_formula(x0.double(), x1.double(), t.double())
    x32 = torch.lerp(x0, x1, t[:, None, None])
    held(c.id, x_path("loss", E, L), "xt", dev, xt_k, xr, x32, scale=xs, group=frames64)
    dr = dsq0.double() + (xr - x1.double()).pow(2).sum((1, 2)) / L
    d32 = dsq0 + (x32 - x1).pow(2).sum((1, 2)) / L
    held(c.id, x_path("loss", E, L), "dsq", dev, dsq_k, dr, d32, extra=fix / dr.abs().clamp_min(1e-300).min())
    for b in range(B):
        if float(t[b]) == 1.0:
            same_bits(c.id, f"xt[{b}] at t = 1 against x1", xt_k[b], x1[b])
            same_bits(c.id, f"dsq[{b}] at t = 1 against its prefill (dsq = 0)", dsq_k[b], dsq0[b])
        if float(t[b]) == 0.0:
            same_bits(c.id, f"xt[{b}] at t = 0 against x0", xt_k[b], x0[b])
    # loss_grad, on the xt and dsq it was handed
    ref = loss_grad_formula(xt_k, x1, u, v, dsq_k, sums0, osl_w, del_w, torch.float64)
    r32 = loss_grad_formula(xt_k, x1, u, v, dsq_k, sums0, osl_w, del_w, torch.float32)
    if osl_w or del_w:
        held(c.id, x_path("loss", E, L), "dv", dev, dv_k, ref[0], r32[0], scale=ref[1], group=frames64)
    held(c.id, x_path("loss", E, L), "sums", dev, sums_k, ref[2], r32[2], scale=ref[3], group=lambda e: e.amax(0), extra=fix / float(ref[3].min()))
    # loss_finalize, on the sums it was handed
    fo, fs, fdu = finalize_formula(sums_k, dsq_k, u, osl_w, del_w, torch.float64)
    fo32, _, fdu32 = finalize_formula(sums_k, dsq_k, u, osl_w, del_w, torch.float32)
    held(c.id, lane_path("loss", B), "out", dev, out_k, fo, fo32, scale=fs, group=lambda e: e)
    held(c.id, lane_path("loss", B), "du", dev, du_k, fdu, fdu32)
    # the formulas are the gradients of the written-out loss (fp64 autograd; sums without prefill)
    vv, uu = v.double().requires_grad_(), u.double().requires_grad_()
    den = dsq_k.double() + C0
    s1 = (xt_k.double() - uu[:, None, None] * vv - x1.double()).pow(2).sum((1, 2)) / L
    s2 = (vv - (xt_k.double() - x1.double()) / den.sqrt()[:, None, None]).pow(2).sum((1, 2)) / L
    (osl_w * (s1 / den).mean() + del_w * s2.mean()).backward()
    z = loss_grad_formula(xt_k, x1, u, v, dsq_k, torch.zeros(B, 3), osl_w, del_w, torch.float64)
    assert float(rel(ref[0], vv.grad, ref[1]).max()) < 1e-12
    assert float(rel(finalize_formula(z[2], dsq_k, u, osl_w, del_w, torch.float64)[2], uu.grad, osl_w / (B * den) * z[3][:, 2] + 1e-300).max()) < 1e-12


ETA_BS = (1, 64, 65, 130)
REACHED |= {lane_path("eta", B) for B in ETA_BS}


def eta_formula(u, num_steps, dt):
    T = lambda s: torch.tensor(s, dtype=dt)      # noqa: E731
    s = u.to(dt).sum() / u.numel()
    r = T(C0).sqrt()
    thr = r + T(f32(1e-6))
    u0 = s if bool(s > thr) else thr
    ratio = (r / u0) ** (T(1.0) / T(float(num_steps)))
    return torch.stack([T(1.0) - ratio, s]), torch.stack([T(1.0) + ratio, u.to(dt).abs().sum() / u.numel()])


def eta_u(kind, B, g):
    r = math.sqrt(C0)
    mean = {"above": 3 * r, "gap": r + 5e-7, "below": 0.3 * r}[kind]
    spread = 0.0 if kind == "gap" else 0.2 * mean
    return (mean + spread * (2 * torch.rand(B, generator=g) - 1)).float()


@pytest.mark.parametrize("num_steps", (1, 8, 50))
@pytest.mark.parametrize("kind", ("above", "gap", "below"))
@pytest.mark.parametrize("B", ETA_BS)
def test_sampler_eta(dev, B, kind, num_steps):
    case = f"eta-{kind}-{B}-{num_steps}"
    u = eta_u(kind, B, gen(B + num_steps))
    eta = Flat((2,), dev)
    ops.sampler_eta(poisoned(u, dev), eta.v, C0, num_steps)
    eta.check(case, "eta")
    ref, sc = eta_formula(u, num_steps, torch.float64)
    r32, _ = eta_formula(u, num_steps, torch.float32)
    held(case, lane_path("eta", B), "eta", dev, eta.v, ref, r32, scale=sc, group=lambda e: e)       # 1 - ratio cancels: against 1 + ratio
    if kind != "above":                      # the clamp: mean(u) at or under sqrt(c0) + 1e-6 steps as if it were there
        thr = torch.tensor(C0).sqrt() + torch.tensor(f32(1e-6))
        exp = 1.0 - (torch.tensor(C0).sqrt().double() / thr.double()) ** (1.0 / num_steps)
        assert abs(float(eta.v[0]) - float(exp)) <= FLOOR * 2


@pytest.mark.parametrize("num_steps", (1, 8, 50))
def test_sampler_eta_groups(dev, num_steps):
    """Songs of 1, 64 and 65 rows (and the kinds of mean above): a song's eta is bit for bit its own od_sampler_eta's."""
    sizes, kinds = (1, 64, 65, 65, 1, 64), ("above", "gap", "below", "above", "below", "above")
    us = [eta_u(k, n, gen(n + i)) for i, (n, k) in enumerate(zip(sizes, kinds))]
    offs = torch.tensor([0] + list(torch.tensor(sizes).cumsum(0)), dtype=torch.int32)
    eta = Flat((len(sizes), 2), dev)
    ops.sampler_eta_groups(poisoned(torch.cat(us), dev), poisoned(offs, dev), eta.v, C0, num_steps)
    eta.check("eta-groups", "eta")
    for i, u in enumerate(us):
        own = Flat((2,), dev)
        ops.sampler_eta(poisoned(u, dev), own.v, C0, num_steps)
        same_bits(f"eta-groups-{num_steps}", f"song {i} ({sizes[i]} rows, {kinds[i]}) against its own od_sampler_eta", eta.v[i], own.v)
    raises(ERR_ARG, lambda: _lib.lib().od_sampler_eta_groups(eta.v.data_ptr(), None, eta.v.data_ptr(), 1, C0, 1, 0))
    raises(ERR_ARG, lambda: _lib.lib().od_sampler_eta_groups(eta.v.data_ptr(), eta.v.data_ptr(), eta.v.data_ptr(), 0, C0, 1, 0))


def group_offs(B, layout):
    """Three songs (one per row when B <= 3: every row is then a boundary).  Larger B: a one-row song first and a two-row song last
    (layout 0), or a one-row song in the middle (layout 1): songs of one row, boundaries at rows 1, B // 2, B // 2 + 1 and B - 2."""
    if B <= 3:
        return list(range(B + 1))
    return [0, 1, B - 2, B] if layout == 0 else [0, B // 2, B // 2 + 1, B]


@pytest.mark.parametrize("layout", (0, 1))
@pytest.mark.parametrize("BL", LOSS_SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_sampler_step(dev, BL, layout):
    """`layout` picks the songs' boundaries and rotates lens by two, so every shape (the two rows of the cap shape too) meets lens of
    0, 1, L - 1 and L."""
    B, L = BL
    case = f"step-{B}x{L}-{layout}"
    g = gen(B + L)
    x, v, u = torch.randn(B, E, L, generator=g), torch.randn(B, E, L, generator=g), 0.1 + torch.rand(B, generator=g)
    eta = torch.tensor([0.37, 123.0])
    xb, vd = Flat((B, E, L), dev, fill=x), poisoned(v, dev)
    ops.sampler_step(xb.v, poisoned(u, dev), vd, poisoned(eta, dev))
    xb.check(case, "x")
    k = (eta[0].double() * u.double())[:, None, None]
    k32 = (eta[0] * u)[:, None, None]
    held(case, x_path("step", E, L), "x", dev, xb.v, x.double() - k * v.double(), x - k32 * v, scale=x.abs() + (k * v.double()).abs(), group=frames64)
    same_bits(case, "v (read only)", vd, v)
    # varlen: every song its own eta (a factor of 10 apart), lens from {0, 1, L - 1, L}; frames at or past lens[b] come out exactly 0
    offs = group_offs(B, layout)
    G = len(offs) - 1
    etas = torch.tensor([[0.5 * 10.0 ** -i, 77.0] for i in range(G)])
    lens = torch.tensor([(0, 1, L - 1, L)[(b + 3 + 2 * layout) % 4] for b in range(B)], dtype=torch.int32).clamp(0, L)
    song = torch.tensor([max(i for i in range(G) if offs[i] <= b) for b in range(B)])
    xb = Flat((B, E, L), dev, fill=x)
    ops.sampler_step_varlen(xb.v, poisoned(u, dev), vd, poisoned(etas, dev), poisoned(lens, dev), poisoned(torch.tensor(offs, dtype=torch.int32), dev))
    xb.check(case, "x (varlen)")
    live = (torch.arange(L)[None, None, :] < lens[:, None, None]).expand(B, E, L)
    k = (etas[song, 0].double() * u.double())[:, None, None]
    k32 = (etas[song, 0] * u)[:, None, None]
    ref = torch.where(live, x.double() - k * v.double(), torch.zeros(1, dtype=torch.float64))
    r32 = torch.where(live, x - k32 * v, torch.zeros(1))
    held(case, x_path("step_varlen", E, L), "x", dev, xb.v, ref, r32, scale=x.abs() + (k * v.double()).abs(), group=frames64)
    assert bool((xb.v.cpu()[~live] == 0).all()), f"{case}: frames at or past lens[b] must be exactly 0"
    if B == 3 and layout == 0:
        n = poisoned(lens, dev)
        raises(ERR_ARG, lambda: _lib.lib().od_sampler_step_varlen(xb.v.data_ptr(), n.data_ptr(), n.data_ptr(), n.data_ptr(), None, n.data_ptr(), 1, B, E, L, 0))
        raises(ERR_ARG, lambda: _lib.lib().od_sampler_step_varlen(xb.v.data_ptr(), n.data_ptr(), n.data_ptr(), n.data_ptr(), n.data_ptr(), n.data_ptr(), 0, B, E, L, 0))


# ================================================================ small linears and packing
LS_SHAPES = ((1, 1, 1), (32, 8, 256), (33, 9, 257), (70, 41, 513), (5, 96, 512))
LS_FAMS = ("random", "row_scale", "cancel", "silu_extreme")
REACHED |= {f"ls_fwd/kc{cdiv(K, LS_KC)}" for _, _, K in LS_SHAPES} | {f"ls_dx/nr{cdiv(N, LS_NR)}" for _, N, _ in LS_SHAPES} | {"ls_dw" for B, _, _ in LS_SHAPES if B > 4}          # the four-way unrolled batch loop of linear_small_dw_kernel


def silu_f(x):
    return x / (1 + (-x).exp())


def silu_grad_f(x):
    s = 1 / (1 + (-x).exp())
    return s * (1 + x * (1 - s))


def silu_grad_terms(x):
    """|terms| of silu_grad: s (1 + x (1 - s)) crosses zero at x = -1.278."""
    s = 1 / (1 + (-x).exp())
    return s * (1 + (x * (1 - s)).abs())


@dataclass(frozen=True)
class LS:
    B: int
    N: int
    K: int
    act: int
    fam: str = "random"
    opt: int = 0         # rotates bias / pre NULL, dW / db NULL, dx NULL / accumulating / overwriting
    det: bool = False

    @property
    def id(self):
        return f"ls-{'silu' if self.act else 'none'}-{self.fam}-o{self.opt}{'-det' if self.det else ''}-{self.B}x{self.N}x{self.K}"


LS_CASES = ([LS(*s, act, "random", i + act) for i, s in enumerate(LS_SHAPES) for act in (OD_ACT_NONE, OD_ACT_SILU)]
            + [LS(*s, act, f, j) for s in ((33, 9, 257), (70, 41, 513)) for j, f in enumerate(LS_FAMS[1:]) for act in (OD_ACT_NONE, OD_ACT_SILU)]
            + [LS(70, 41, 513, OD_ACT_SILU, "random", o) for o in (0, 1, 2, 3, 4, 5)]
            + [LS(*s, OD_ACT_SILU, "random", o, True) for s in ((70, 41, 513), (5, 96, 512)) for o in (1, 2)])
LS_CASES = list(dict.fromkeys(LS_CASES))


def ls_inputs(c, g):
    B, N, K = c.B, c.N, c.K
    x, W, b = torch.randn(B, K, generator=g), torch.randn(N, K, generator=g) / math.sqrt(K), 0.5 * torch.randn(N, generator=g)
    dout = torch.randn(B, N, generator=g)
    if c.fam == "row_scale":
        s = (10.0 ** (torch.arange(B) % 3).float())[:, None]
        x, dout = x * s, dout * s
    elif c.fam == "cancel":                  # x's columns equal in pairs, W's opposite: every forward sum cancels to 1e-3 of its terms;
        K2, N2 = K // 2, N // 2              # W's rows opposite in pairs, dout's equal: so does every sum of dx
        x[:, 1:2 * K2:2] = x[:, 0:2 * K2:2]
        W[:, 1:2 * K2:2] = -W[:, 0:2 * K2:2] * (1 + 1e-3 * torch.randn(N, K2, generator=g))
        W[1:2 * N2:2] = -W[0:2 * N2:2]
        dout[:, 1:2 * N2:2] = dout[:, 0:2 * N2:2] * (1 + 1e-3 * torch.randn(B, N2, generator=g))
        b = b * 1e-3
    elif c.fam == "silu_extreme":            # pre-activations of +-30 .. +-1e4
        W = W * 1e-2
        b = (2 * torch.randint(0, 2, (N,), generator=g) - 1).float() * 30 * 10.0 ** (2.5 * torch.rand(N, generator=g))
    return x, W, b, dout


def tile_max(t, tr, tc, sum_=False):
    """Largest element (or the sum) of every (tr x tc) tile of the matrix t >= 0 (ragged last tiles)."""
    M, N = t.shape
    tm, tn = cdiv(M, tr), cdiv(N, tc)
    p = torch.nn.functional.pad(t.double(), (0, tn * tc - N, 0, tm * tr - M)).reshape(tm, tr, tn, tc)
    return p.sum((1, 3)) if sum_ else p.amax((1, 3))


def small_tiles(M, N, tr, tc, least):
    """(M, N) mask of the elements whose (tr x tc) tile holds fewer than `least` elements (ragged corner tiles)."""
    rows = torch.tensor([min(tr, M - r // tr * tr) for r in range(M)])
    cols = torch.tensor([min(tc, N - c // tc * tc) for c in range(N)])
    return rows[:, None] * cols[None, :] < least


def silu_floor(pre, tr, tc):
    """(8 + max(-x, 0)) eps per tile, -x counted up to 89 (past it exp(-x) is Inf in fp32 and the result exact): the module docstring's
    exception.  Positive x keeps 8 eps: there exp(-x) is small beside 1 and its error does not show."""
    return (8 + tile_max((-pre).clamp(0.0, 89.0), tr, tc)) * EPS32


def held_tiles(case, row, what, device, tr, tc, out, ref, ref32, scale=None, extra=0.0, floor=FLOOR):
    """held() in relative L2 per (tr x tc) tile, with no denominator floors: every tile counts."""
    ek, e32 = (tile_errors(t, ref, tr, tc, floor=0.0, scale=scale, floor_max=0.0)[0] for t in (out.cpu(), ref32))
    ek = torch.nan_to_num(ek, nan=INF)
    bound = torch.maximum(4 * e32, torch.as_tensor(floor, dtype=torch.float64).expand_as(e32)) + extra
    w = int((ek / bound).flatten().argmax())
    print(f"MEASURED {row} {what} {'hip' if device.type == 'cuda' else 'emu'} {float(ek.flatten()[w]):.3e} {float(bound.flatten()[w]):.3e} {case}")
    assert float((ek / bound).flatten()[w]) <= 1.0, (f"{case} {what}: tile {w} of {tuple(ek.shape)} error {float(ek.flatten()[w]):.3e} > bound "
                                                      f"{float(bound.flatten()[w]):.3e} (fp32 torch {float(e32.flatten()[w]):.3e})")


@pytest.mark.parametrize("c", LS_CASES, ids=lambda c: c.id)
def test_linear_small(dev, c):
    B, N, K = c.B, c.N, c.K
    x, W, b, dout = ls_inputs(c, gen(B + 7 * N + 13 * K + c.act))
    no_bias, no_pre = c.opt % 3 == 1, c.opt % 3 == 2 and not c.act          # the backward of SiLU needs pre
    dw_on, db_on = c.opt % 4 != 1, c.opt % 4 != 2
    dx_mode = ("overwrite", "accumulate", "none")[c.opt % 3]
    if c.det:
        dx_mode = ("overwrite", "accumulate")[c.opt % 2]
    xd, Wd, bd = poisoned(x, dev), poisoned(W, dev), None if no_bias else poisoned(b, dev)
    out, pre = Flat((B, N), dev), None if no_pre else Flat((B, N), dev)
    ops.linear_small(xd, Wd, bd, out.v, None if pre is None else pre.v, c.act)
    out.check(c.id, "out")
    x64, W64, b64 = x.double(), W.double(), torch.zeros(N, dtype=torch.float64) if no_bias else b.double()
    b32 = torch.zeros(N) if no_bias else b
    pr = x64 @ W64.T + b64
    pr32 = x @ W.T + b32
    # tiles are measured against their reference's own norm; against sum |x| |W| + |bias| in the cancelling family, and in the ragged corner
    # tiles of fewer than 8 elements (1 at B 33, N 9; 6 at B 70, N 41): one element's error relative to its own value, a sum of K signed
    # terms, is 4 x another summation order's only on average
    terms = x64.abs() @ W64.abs().T + b64.abs()
    cancel = c.fam == "cancel"
    sc = terms if cancel else torch.where(small_tiles(B, N, 32, LS_NB, 8), terms, pr.abs())
    fwd = f"ls_fwd/kc{cdiv(K, LS_KC)}"
    if pre is not None:
        pre.check(c.id, "pre")
        held_tiles(c.id, fwd, "pre", dev, 32, LS_NB, pre.v, pr, pr32, sc)
    if c.act:
        assert not bool(torch.isnan(out.v).any())
        pk = pre.v.cpu()                     # out = silu(s) of the very s that went to pre
        held_tiles(c.id, fwd, "out", dev, 32, LS_NB, out.v, silu_f(pk.double()), silu_f(pk), silu_f(pk.double()).abs() + TINY, floor=silu_floor(pk, 32, LS_NB))
    else:
        held_tiles(c.id, fwd, "out", dev, 32, LS_NB, out.v, pr, pr32, sc)
    # backward, on the pre the forward wrote (or none: no activation)
    pre_k = None if pre is None else pre.v.cpu()
    dW0, db0, dx0 = torch.randn(N, K, generator=gen(1)), torch.randn(N, generator=gen(2)), torch.randn(B, K, generator=gen(3))
    runs = []
    for _ in range(2 if c.det else 1):
        dpre = Flat((B, N), dev)
        dW, db = Flat((N, K), dev, fill=dW0) if dw_on else None, Flat((N,), dev, fill=db0) if db_on else None
        dx = None if dx_mode == "none" else Flat((B, K), dev, fill=dx0 if dx_mode == "accumulate" else None)
        det_run(dev, c.det, [dx.v] if c.det else [], lambda: ops.linear_small_bwd(
            xd, Wd, None if pre is None else pre.v, poisoned(dout, dev), dpre.v, None if dW is None else dW.v, None if db is None else db.v,
            None if dx is None else dx.v, dx_mode == "accumulate", c.act))
        runs.append((dpre, dW, db, dx))
    if c.det:
        same_bits(c.id, "dx of two deterministic runs", runs[0][3].v, runs[1][3].v)
    dpre, dW, db, dx = runs[0]
    dpre.check(c.id, "dpre")
    do64 = dout.double()
    dp = do64 * silu_grad_f(pre_k.double()) if c.act else do64
    dp32 = dout * silu_grad_f(pre_k) if c.act else dout
    held_tiles(c.id, "ls_dw", "dpre", dev, 32, LS_NB, dpre.v, dp, dp32, do64.abs() * silu_grad_terms(pre_k.double()) + TINY if c.act else None,
               floor=silu_floor(pre_k, 32, LS_NB) if c.act else FLOOR)
    dpk = dpre.v.cpu()                       # dW, db and dx read the dpre the first kernel wrote
    if dW is not None:
        dW.check(c.id, "dW")
        wr, wt = dW0.double() + dpk.double().T @ x64, dW0.double().abs() + dpk.double().abs().T @ x64.abs()
        held_tiles(c.id, "ls_dw", "dW", dev, 1, 256, dW.v, wr, dW0 + dpk.T @ x, wt if cancel else torch.where(small_tiles(N, K, 1, 256, 8), wt, wr.abs()))
    if db is not None:
        db.check(c.id, "db")
        held(c.id, "ls_dw", "db", dev, db.v, db0.double() + dpk.double().sum(0), db0 + dpk.sum(0), scale=db0.abs() + dpk.double().abs().sum(0))
    if dx is not None:
        dx.check(c.id, "dx")
        old = dx0.double() if dx_mode == "accumulate" else torch.zeros(B, K, dtype=torch.float64)
        dsc = old.abs() + dpk.double().abs() @ W64.abs()
        # deterministic mode: every 32-row slice of N adds one fixed-point value per element, each within 2^-41 of its fp32 value
        xr = old + dpk.double() @ W64
        xs = dsc if cancel else torch.where(small_tiles(B, K, 32, 256, 8), dsc, xr.abs())
        # in L2 over a tile of n elements that is sqrt(n) slices 2^-41 against the tile's norm
        fix = cdiv(N, LS_NR) * FIX * tile_max(torch.ones(B, K), 32, 256, sum_=True).sqrt() / tile_max(xs.pow(2), 32, 256, sum_=True).sqrt() if c.det else 0.0
        held_tiles(c.id, f"ls_dx/nr{cdiv(N, LS_NR)}", "dx", dev, 32, 256, dx.v, xr, old.float() + dpk @ W, xs, extra=fix)
    same_bits(c.id, "W (read only)", Wd, W)


PACK_SHAPES = ((10, 6, 16, 8), (1, 1, 8, 32), (33, 70, 40, 96))
PACK_TS, PACK_TR = ("bf16", "fp32", "split"), (False, True)
REACHED |= {f"pack/{T}{'/t' if tr else ''}" for T in PACK_TS[:2] for tr in PACK_TR} | {"pack/split" for N, K, Np, Kp in PACK_SHAPES if Kp % 32 == 0 and "split" in PACK_TS}


def row_map_of(N, Np, g):
    """Every kind of entry: -1 (a zero row), repeated sources, the identity."""
    rm = torch.randint(0, N, (Np,), generator=g, dtype=torch.int32)
    rm[::3] = -1
    if Np > 4:
        rm[4] = rm[1]
    return rm


@pytest.mark.parametrize("mapped", (False, True), ids=("plain", "row_map"))
@pytest.mark.parametrize("T", PACK_TS)
@pytest.mark.parametrize("shape", PACK_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_pack_weight(dev, shape, T, mapped):
    N, K, Np, Kp = shape
    case = f"pack-{T}-{shape}-{mapped}"
    g = gen(N + K)
    src = torch.randn(N, K, generator=g) * 2.0 ** torch.randint(-8, 9, (N, K), generator=g).float()
    rm = row_map_of(N, Np, g) if mapped else None
    rows = rm.long() if mapped else torch.cat([torch.arange(N), torch.full((Np - N,), -1)])
    full = torch.zeros(Np, Kp)
    full[rows >= 0, :K] = src[rows[rows >= 0]]
    sd, rd = poisoned(src, dev), None if rm is None else poisoned(rm, dev)
    if T == "split":
        st = Flat((Np, Kp), dev)
        if Kp % 32:
            raises(ERR_UNSUPPORTED, lambda: ops.pack_weight(sd, ops.SplitWeight(st.v), row_map=rd))
            assert bool(torch.isnan(st.buf).all())
            return
        ops.pack_weight(sd, ops.SplitWeight(st.v), row_map=rd)
        assert bool(torch.isnan(st.buf[:64]).all() & torch.isnan(st.buf[64 + st.n:]).all()), f"{case}: written outside dst"
        h = st.v.cpu().view(torch.bfloat16).reshape(Np, Kp // 32, 2, 32)          # [n][slab][hi / lo][j]: dst[n][32 s + j] and + 32, as bf16 slots
        hi, lo = h[:, :, 0].reshape(Np, Kp), h[:, :, 1].reshape(Np, Kp)
        same_bits(case, "hi (the bf16 rounding)", hi, full.to(torch.bfloat16))
        same_bits(case, "lo (the bf16 rounding of the remainder)", lo, (full - full.to(torch.bfloat16).float()).to(torch.bfloat16))
        err = (hi.double() + lo.double() - full.double()).abs()
        assert bool((err <= 2.0 ** -16 * full.double().abs()).all()), f"{case}: hi + lo is off by {float((err / full.abs().clamp_min(1e-30)).max()):.3e}"
        assert bool((hi[full == 0].float() == 0).all() & (lo[full == 0].float() == 0).all()), f"{case}: padding must be exactly 0"
        raises(ERR_UNSUPPORTED, lambda: _lib.lib().od_pack_weight(_lib.OD_F32X3W, sd.data_ptr(), N, K, st.v.data_ptr(), Np, Kp, 1, None, 0))
        return
    dt = {"bf16": torch.bfloat16, "fp32": torch.float32}[T]
    for tr in PACK_TR:
        dst = Flat((Kp, Np) if tr else (Np, Kp), dev, dtype=dt)
        ops.pack_weight(sd, dst.v, transpose=tr, row_map=rd)
        dst.check(case, "dst")
        exp = (full.T if tr else full).contiguous().to(dt)
        same_bits(case, f"dst (transpose {tr})", dst.v, exp)
    same_bits(case, "src (read only)", sd, src)


FRAMES_CL = ((1, 130), (63, 65), (64, 64), (65, 63), (130, 1))
SCALE_BLC = ((1, 1, 8), (3, 63, 64), (2, 130, 72))
CAST_NS = (1, 255, 257, 70001)
REACHED |= {"frames" for C, L in FRAMES_CL if C > 64 or L > 64} | {"scale" for B, L, C in SCALE_BLC if B > 1} | {"cast" for n in CAST_NS if n > 256}


@pytest.mark.parametrize("T", ("bf16", "fp32"))
@pytest.mark.parametrize("CL", FRAMES_CL, ids=lambda s: f"{s[0]}x{s[1]}")
def test_cl_to_frames(dev, CL, T):
    C, L = CL
    B = 2
    dt = {"bf16": torch.bfloat16, "fp32": torch.float32}[T]
    src = torch.randn(B, C, L, generator=gen(C + L))
    dst = Fenced(B * L, C, dt, dev)          # ld > C, NaN columns either side and NaN rows below
    ops.cl_to_frames(poisoned(src, dev), dst.v)
    dst.check(f"frames-{T}-{C}x{L}", "dst")
    same_bits(f"frames-{T}-{C}x{L}", "dst", dst.v, src.permute(0, 2, 1).reshape(B * L, C).to(dt))


SILU_NS = (8, 8 * (4096 * 256) + 8)
SPECIAL = (0.0, 88.0, -88.0, 1e4, -1e4, -INF, INF, 1.0)
REACHED |= {flat_path(k, n, 8) for n in SILU_NS for k in ("silu", "silu_bwd")}


@pytest.mark.parametrize("T", ("bf16", "fp32"))
@pytest.mark.parametrize("n", SILU_NS)
def test_silu(dev, n, T):
    """od_silu / od_silu_bwd.  n = 8: 0, +-88, +-1e4 and +-Inf (the formula's own limits: silu(-Inf) = -Inf / Inf = NaN, as in torch); the large n:
    N(0, 2) with those values at both ends.  The floor is (8 + max(-x, 0)) eps: see the module docstring."""
    dt = {"bf16": torch.bfloat16, "fp32": torch.float32}[T]
    case = f"silu-{T}-{n}"
    g = gen(n % 977)
    x = 2 * torch.randn(n, generator=g)
    x[:8] = torch.tensor(SPECIAL)
    x[-8:] = torch.tensor(SPECIAL).flip(0)
    dy = torch.randn(n, generator=g)
    x, dy = x.to(dt), dy.to(dt)
    xd, dyd = poisoned(x, dev), poisoned(dy, dev)
    y, dx = Flat((n,), dev, dtype=dt), Flat((n,), dev, dtype=dt)
    ops.silu(xd, y.v)
    ops.silu_bwd(xd, dyd, dx.v)
    x64, x32 = x.double(), x.float()
    ry, rdx = silu_f(x64), dy.double() * silu_grad_f(x64)
    terms = torch.nan_to_num(dy.double().abs() * silu_grad_terms(x64), nan=0.0)
    for buf, name, ref, r32, sc in ((y, "silu", ry, silu_f(x32), ry.abs()), (dx, "silu_bwd", rdx, dy.float() * silu_grad_f(x32), terms)):
        assert bool(torch.isnan(buf.buf[:64].float()).all() & torch.isnan(buf.buf[64 + n:].float()).all()), f"{case}: written outside {name}"
        assert torch.equal(torch.isnan(buf.v.float()).cpu(), torch.isnan(ref)), f"{case}: {name} is NaN in other places than the formula"
        fin = torch.isfinite(ref)
        inf = torch.isinf(ref)                # silu(+Inf) = +Inf: compared as a value, not only as not-NaN
        assert torch.equal(buf.v.double().cpu()[inf], ref[inf]), f"{case}: {name} at x = {x64[inf].tolist()}: {buf.v.double().cpu()[inf].tolist()}"
        half_ulp = half_ulp_bf16(ref) if T == "bf16" else torch.zeros_like(ref)
        e = (buf.v.double().cpu() - ref).abs()[fin]
        e32 = (r32.double() - ref).abs()[fin]
        lim = torch.maximum(4 * e32, (8 + (-x64).clamp(0.0, 89.0)[fin]) * EPS32 * sc[fin]) + half_ulp[fin] + 1e-45      # 1e-45: below fp32's denormals
        w = int((e / lim).argmax())
        print(f"MEASURED {flat_path(name, n, 8)} {name}-{T} {'hip' if dev.type == 'cuda' else 'emu'} {float(e[w] / ref.abs()[fin][w].clamp_min(1e-300)):.3e} "
              f"{float(lim[w] / ref.abs()[fin][w].clamp_min(1e-300)):.3e} {case}")
        assert bool((e <= lim).all()), f"{case} {name}: x = {float(x64[fin][w])}: {float(buf.v.double().cpu()[fin][w])} against {float(ref[fin][w])} (limit {float(lim[w]):.3e})"
    lib = _lib.lib()
    for bad in (7, 12):
        raises(ERR_ALIGN, lambda: lib.od_silu(ops.dt_code(dt), xd.data_ptr(), y.v.data_ptr(), bad, 0))
        raises(ERR_ALIGN, lambda: lib.od_silu_bwd(ops.dt_code(dt), xd.data_ptr(), dyd.data_ptr(), dx.v.data_ptr(), bad, 0))


@pytest.mark.parametrize("T", ("bf16", "fp32"))
@pytest.mark.parametrize("BLC", SCALE_BLC, ids=lambda s: "x".join(map(str, s)))
def test_scale_channels(dev, BLC, T):
    """Dropout1d's channel factors: exactly 0 and 1 / (1 - p).  One IEEE product per element (then one rounding to bf16): exact."""
    B, L, C = BLC
    dt = {"bf16": torch.bfloat16, "fp32": torch.float32}[T]
    g = gen(B + L + C)
    x = torch.randn(B * L, C, generator=g).to(dt)
    f = torch.where(torch.rand(B, C, generator=g) < 0.3, torch.zeros(1), torch.tensor(1 / (1 - 0.1)))
    xb = Fenced(B * L, C, dt, dev, fill=x.to(dev))
    fd = poisoned(f, dev)
    ops.scale_channels(xb.v, fd, B, L)
    xb.check(f"scale-{T}-{BLC}", "x")
    exp = (x.float() * f.repeat_interleave(L, 0)).to(dt)
    assert torch.equal(xb.v.cpu(), exp), f"scale-{T}-{BLC}: x * scale is one correctly rounded product"
    assert bool((xb.v.cpu()[f.repeat_interleave(L, 0) == 0] == 0).all())
    raises(ERR_ALIGN, lambda: _lib.lib().od_scale_channels(ops.dt_code(dt), xb.v.data_ptr(), xb.buf.stride(0), fd.data_ptr(), B, L, C - 4, 0))


@pytest.mark.parametrize("n", CAST_NS)
def test_cast_rows(dev, n):
    g = gen(n)
    x = torch.randn(n, generator=g) * 2.0 ** torch.randint(-30, 31, (n,), generator=g).float()
    ties = torch.tensor([1 + 2.0 ** -8, 1 + 3 * 2.0 ** -8, -(1 + 2.0 ** -8), -(1 + 3 * 2.0 ** -8), 1 + 2.0 ** -8 + 2.0 ** -23, 1 + 2.0 ** -8 - 2.0 ** -23, 0.0, -0.0])
    x[:min(n, 8)] = ties[:min(n, 8)]
    lo = Flat((n,), dev, dtype=torch.bfloat16)
    ops.cast_rows(poisoned(x, dev), lo.v)
    lo.check(f"cast-{n}", "bf16")
    same_bits(f"cast-{n}", "fp32 -> bf16 (round to nearest even)", lo.v, x.to(torch.bfloat16))
    if n >= 8:                               # ties go to the even neighbour, whichever side it is on
        assert lo.v[:6].float().cpu().tolist() == [1.0, 1 + 2.0 ** -6, -1.0, -(1 + 2.0 ** -6), 1 + 2.0 ** -7, 1.0]
    hi = Flat((n,), dev)
    ops.cast_rows(lo.v, hi.v)
    hi.check(f"cast-{n}", "fp32")
    same_bits(f"cast-{n}", "bf16 -> fp32", hi.v, x.to(torch.bfloat16).float())
    back = Flat((n,), dev, dtype=torch.bfloat16)
    ops.cast_rows(hi.v, back.v)
    same_bits(f"cast-{n}", "bf16 -> fp32 -> bf16", back.v, lo.v)
    raises(ERR_UNSUPPORTED, lambda: _lib.lib().od_cast_rows(_lib.OD_F32, hi.v.data_ptr(), _lib.OD_F32, hi.v.data_ptr(), n, 0))
    raises(ERR_ARG, lambda: _lib.lib().od_cast_rows(_lib.OD_F32, hi.v.data_ptr(), _lib.OD_BF16, lo.v.data_ptr(), 0, 0))


# ================================================================ style forward
STYLE_SHAPES = ((1, 1, 1, 1), (3, 5, 16, 256), (2, 7, 33, 300))
REACHED |= {"style_cond" for *_, H in STYLE_SHAPES if H > 256}          # two blocks in x


def style_formula(labels, rw, rb, cw, cb, nul, dt):
    labels, rw, rb, cw, cb, nul = (t.to(dt) for t in (labels, rw, rb, cw, cb, nul))
    F = rw.numel()
    T = lambda s: torch.tensor(s, dtype=dt)      # noqa: E731
    masked = labels < 0
    lab = torch.where(masked, torch.zeros_like(labels), labels)          # a masked slot's feature is never read
    rff = (T(2.0) / T(float(F))).sqrt() * (lab[:, :, None] / T(10.0) * rw + rb).cos()             # (B, NL, F)
    per = cb[None] + torch.einsum("bnf,nfh->bnh", rff, cw)
    ab = cb.abs()[None] + torch.einsum("bnf,nfh->bnh", rff.abs(), cw.abs())
    m = masked[:, :, None]
    return torch.where(m, nul[None], per).sum(1), torch.where(m, nul.abs()[None], ab).sum(1)


@pytest.mark.parametrize("kind", ("valid", "masked", "mixed", "neg_inf"))
@pytest.mark.parametrize("shape", STYLE_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_style_conditioning(dev, shape, kind):
    B, NL, F, H = shape
    case = f"style_cond-{kind}-{shape}"
    g = gen(B + NL + F + H)
    labels = 10 * torch.rand(B, NL, generator=g)
    if kind == "masked":
        labels[:] = -1.0
    elif kind in ("mixed", "neg_inf"):
        labels[torch.rand(B, NL, generator=g) < 0.4] = -1.0
        labels[0, 0] = -1.0
        if NL > 1:
            labels[0, 1] = 3.0
    if kind == "neg_inf":
        labels[labels < 0] = -INF
    rw, rb = torch.randn(F, generator=g), 6.28 * torch.rand(F, generator=g)
    cw, cb, nul = torch.randn(NL, F, H, generator=g) / math.sqrt(F), torch.randn(NL, H, generator=g), torch.randn(NL, H, generator=g)
    c = Flat((B, H), dev)
    ops.style_conditioning(*(poisoned(t, dev) for t in (labels, rw, rb, cw, cb, nul)), c.v)
    c.check(case, "c")
    ref, sc = style_formula(labels, rw, rb, cw, cb, nul, torch.float64)
    r32, _ = style_formula(labels, rw, rb, cw, cb, nul, torch.float32)
    held(case, "style_cond", "c", dev, c.v, ref, r32, scale=sc, group=lambda e: e.amax(1))


RMS_MS, RMS_CS = (1, 4, 5), (1, 64, 65, 256)
REACHED |= {"rms_rows" for M in RMS_MS if M > 4}         # the second block of four rows


@pytest.mark.parametrize("gamma_on", (False, True), ids=("plain", "gamma"))
@pytest.mark.parametrize("C", RMS_CS)
@pytest.mark.parametrize("M", RMS_MS)
def test_rmsnorm_rows(dev, M, C, gamma_on):
    """Row RMS from 2^-20 to 2^20; with M > 1 row 0 is all zero (it comes out exactly 0), so the only row of M = 1 and the one row of the
    second block at M = 5 carry values.  Every other row against its own reference row."""
    case = f"rms_rows-{M}x{C}-{gamma_on}"
    g = gen(M + C)
    eps = f32(1e-6)
    x = torch.randn(M, C, generator=g) * 2.0 ** torch.linspace(-20, 20, M)[:, None]
    zero = M > 1
    if zero:
        x[0] = 0
    gamma = 1 + 0.5 * torch.randn(C, generator=g) if gamma_on else None
    y = Flat((M, C), dev)
    ops.rmsnorm_rows(poisoned(x, dev), None if gamma is None else poisoned(gamma, dev), y.v, eps)
    y.check(case, "y")

    def formula(dt):
        xx = x.to(dt)
        r = xx * (xx.pow(2).sum(1, keepdim=True) / C + torch.tensor(eps, dtype=dt)).rsqrt()
        return r if gamma is None else r * gamma.to(dt)
    ref = formula(torch.float64)
    if zero:
        assert bool((y.v[0] == 0).all()), f"{case}: the all-zero row"
    ek, e32 = (tile_errors(t, ref, 1, C, floor=0.0, floor_max=0.0)[0].flatten()[int(zero):] for t in (y.v.cpu(), formula(torch.float32)))
    assert ek.numel() == M - int(zero) >= 1
    bound = (4 * e32).clamp_min(FLOOR)
    print(f"MEASURED rms_rows y {'hip' if dev.type == 'cuda' else 'emu'} {float(ek.max()):.3e} {float(bound[ek.argmax()]):.3e} {case}")
    assert bool((ek <= bound).all()), f"{case}: row errors {ek.tolist()} > {bound.tolist()}"


# ================================================================ deterministic accumulation
DET_NS = (4, 4096 * 256 + 77)
REACHED |= {"det/small" if cdiv(n, 256) <= CAP_1D else "det/cap" for n in DET_NS}


def red_add(device, dst, value):
    """One od_red_add of `value` (a square, as fp32) into dst[0]: od_make_xt at E = L = 1, t = 0 adds (x0 - x1)^2 / 1, one block-sum per launch."""
    r = math.sqrt(value)
    assert f32(r) == r and f32(r * r) == value
    xt = Flat((1, 1, 1), device)
    ops.make_xt(poisoned(torch.tensor([[[r]]]), device), poisoned(torch.zeros(1, 1, 1), device), poisoned(torch.zeros(1), device), xt.v, dst)
    assert float(xt.v) == r


@pytest.fixture
def det_ctx(dev):
    try:
        det.force(True)
        yield det.context(dev)
    finally:
        det.force(None)


def test_det_exact_and_order_free(dev, det_ctx):
    """Multiples of 2^-40 add up exactly through the shadow, in either launch order; the flush folds the shadow in and zeroes it; a sub-range
    flush folds only that sub-range."""
    ks = (1, 3, 5, 1023, 2049)               # (k 2^-20)^2 = k^2 2^-40
    results = []
    for order in (ks, ks[::-1]):
        buf = Flat((4,), dev, fill=torch.tensor([0.0, 0.5, -0.25, 0.0]))
        det_ctx.register(buf.v)
        for i in range(4):
            for k in (ks[:i + 2] if order is ks else ks[:i + 2][::-1]):
                red_add(dev, buf.v[i:i + 1], (k * 2.0 ** -20) ** 2)
        same_bits("det", "the destinations before any flush", buf.v, torch.tensor([0.0, 0.5, -0.25, 0.0]))
        det_ctx.flush(buf.v[1:3])
        part = buf.v.clone()
        det_ctx.flush(buf.v)
        full = buf.v.clone()
        det_ctx.flush(buf.v)
        same_bits("det", "a second flush (the first zeroed the shadow)", buf.v, full)
        buf.check("det", "dst")
        results.append((part, full, order))
    for part, full, order in results:
        sums = torch.tensor([sum(k * k for k in ks[:i + 2]) * 2.0 ** -40 for i in range(4)], dtype=torch.float64)
        assert torch.equal(sums.float().double(), sums), "the sums are fp32 numbers: the flush adds them with one fp32 rounding (none into 0)"
        exp = torch.tensor([0.0, 0.5, -0.25, 0.0]) + sums.float()
        same_bits("det", "the flushed sums", full, exp)
        same_bits("det", "a flush of [1, 3) alone", part, torch.tensor([0.0, float(exp[1]), float(exp[2]), 0.0]))
    same_bits("det", "the two launch orders", results[0][1], results[1][1])


def test_det_format_limits(dev, det_ctx):
    """Under 2^-41 a contribution rounds to no step at all; from 2^23 on it bypasses the shadow and lands in the destination at once."""
    buf = Flat((3,), dev, fill=torch.tensor([1.0, 1.0, 1.0]))
    det_ctx.register(buf.v)
    red_add(dev, buf.v[0:1], 2.0 ** -42)     # < 2^-41: llrint(0.25) = 0
    red_add(dev, buf.v[1:2], 2.0 ** 24)      # >= 2^23: a plain atomic
    red_add(dev, buf.v[2:3], 2.0 ** -40)     # one step
    same_bits("det", "before the flush: only the large value has landed", buf.v, torch.tensor([1.0, 1.0 + 2.0 ** 24, 1.0]))
    det_ctx.flush(buf.v)
    same_bits("det", "after the flush", buf.v, torch.tensor([1.0, 1.0 + 2.0 ** 24, 1.0]))          # 1 + 2^-40 rounds to 1 in fp32
    buf.v.zero_()
    red_add(dev, buf.v[0:1], 2.0 ** -42)
    red_add(dev, buf.v[2:3], 2.0 ** -40)
    det_ctx.flush(buf.v)
    same_bits("det", "into zero: the sub-step value is gone, one step is 2^-40", buf.v, torch.tensor([0.0, 0.0, 2.0 ** -40]))
    raises(ERR_ARG, lambda: det_ctx.flush(torch.zeros(4, device=dev)))             # not a registered range


def test_det_flush_past_the_grid_cap(dev, det_ctx):
    n = DET_NS[1]
    fill = torch.randn(n, generator=gen(3))
    buf = Flat((n,), dev, fill=fill)
    det_ctx.register(buf.v)
    spots = (0, 255, 256, 4096 * 256 - 1, 4096 * 256, n - 1)
    for i in spots:
        buf.v[i] = 0.0
        red_add(dev, buf.v[i:i + 1], 2.0 ** -20)
    det_ctx.flush(buf.v)
    exp = fill.clone()
    exp[list(spots)] = 2.0 ** -20
    buf.check("det-cap", "dst")
    same_bits("det-cap", "a flush of more than 4096 256 elements", buf.v, exp)


# ================================================================ the table
def test_step_dispatch_table_matches_sources():
    """The constants the path functions mirror are the ones in the sources, and the cases of this file reach every row of the table — on
    the emulator too, except GPU_ONLY_ROWS.  A failure here names the constant: resize the case that was built on it (SQ_NS, ADAM_NS,
    LOSS_SHAPES, ETA_BS, LS_SHAPES, SILU_NS, DET_NS)."""
    optim, heads, misc, style, detc = (open(os.path.join(CSRC, f)).read() for f in ("optim.hip", "heads.hip", "misc.hip", "style.hip", "det.hip"))
    assert f"constexpr int SQ_MAX_BLOCKS = {SQ_MAX_BLOCKS};" in optim, "SQ_MAX_BLOCKS: resize SQ_NS"
    assert "int blocks = (int)((n / 4 + 255) / 256); if (blocks > SQ_MAX_BLOCKS) blocks = SQ_MAX_BLOCKS; if (blocks < 1) blocks = 1;" in optim
    assert optim.count(f"int blocks = (int)((n + 255) / 256); if (blocks > {CAP_1D}) blocks = {CAP_1D};") == 2, "adamw / ema grid cap: resize ADAM_NS"
    assert misc.count(f"long n8 = n / 8; int blocks = (int)((n8 + 255) / 256); if (blocks > {CAP_1D}) blocks = {CAP_1D}; if (blocks < 1) blocks = 1;") == 2, \
        "silu grid cap: resize SILU_NS"
    assert f"int blocks = (int)((count + 255) / 256); if (blocks > {CAP_1D}) blocks = {CAP_1D};" in detc, "det_flush grid cap: resize DET_NS"
    assert heads.count(f"int gx = (EL + 255) / 256; if (gx > {CAP_X}) gx = {CAP_X};") == 4, "make_xt / loss_grad / sampler_step grid cap: resize LOSS_SHAPES"
    assert heads.count(f"b += {LANES}) ") >= 3 and "for (int b = lane; b < n; b += 64) s += u[r0 + b];" in heads, "64-lane loops: resize ETA_BS and LOSS_SHAPES"
    assert f"constexpr int LS_KC = {LS_KC}, LS_NB = {LS_NB};" in misc and f"constexpr int LS_NR = {LS_NR};" in misc, "LS_*: resize LS_SHAPES"
    assert "dim3((N + LS_NB - 1) / LS_NB, (B + 31) / 32)" in misc and "dim3((N + LS_NR - 1) / LS_NR, (B + 31) / 32, (K + 255) / 256)" in misc
    assert "dim3((K + 255) / 256, N)" in misc
    assert f"constexpr int SC_FT = {SC_FT}, SC_BS = {SC_BS};" in style
    assert "dim3((H + 255) / 256, B)" in style and "dim3((M + 3) / 4)" in style
    assert "if (det && fabsf(v) < 8388608.f) {" in open(os.path.join(CSRC, "od_common.h")).read()      # 2^23: the shadow's upper limit
    assert len(set(ROWS)) == len(ROWS)
    assert REACHED == set(ROWS), (sorted(REACHED - set(ROWS)), sorted(set(ROWS) - REACHED))
    assert GPU_ONLY_ROWS == []               # every case takes the `dev` fixture: both backends run all of them
    # the shapes sit where the issue puts them: one over a cap, one under
    assert cdiv(SQ_NS[5] // 4, 256) == SQ_MAX_BLOCKS + 1 and cdiv(SQ_NS[6] // 4, 256) > 2 * SQ_MAX_BLOCKS and cdiv(SQ_NS[4] // 4, 256) == 3
    assert cdiv(ADAM_NS[3], 256) == CAP_1D + 1 and cdiv(SILU_NS[1] // 8, 256) == CAP_1D + 1 and cdiv(DET_NS[1], 256) == CAP_1D + 1
    assert cdiv(E * LOSS_SHAPES[3][1], 256) == CAP_X + 1 and LOSS_SHAPES[2][0] > LANES
    assert {cdiv(B, LANES) for B in ETA_BS} == {1, 2, 3} and {B % LANES for B in ETA_BS} >= {0, 1}
    assert {(cdiv(B, 32), B % 32 != 0) for B, _, _ in LS_SHAPES} >= {(1, False), (2, True), (3, True)}
    assert {K % LS_KC for _, _, K in LS_SHAPES} >= {0, 1} and {N % LS_NB != 0 for _, N, _ in LS_SHAPES} == {True, False}
    assert {v for CL in FRAMES_CL for v in CL} >= {1, 63, 64, 65, 130} and {M % 4 for M in RMS_MS} >= {0, 1} and {C % 64 for C in RMS_CS} >= {0, 1}
    assert any(H > 256 for *_, H in STYLE_SHAPES) and any(F > SC_FT and F % SC_FT for _, _, F, _ in STYLE_SHAPES)

