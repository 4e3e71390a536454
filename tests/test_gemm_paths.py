"""Every GEMM kernel the library dispatches, against an fp64 reference computed from the same rounded operands, tile by tile (the kernel's
own output tile), on inputs built to reach the places where a tiled, pipelined GEMM goes wrong.

Dispatch table (osu_dreamer_amd/csrc/gemm.hip: launch_nt, launch_tn, od_gemm_nt, od_gemm_nt_qkrope, od_gemm_nt_qkrope_split, od_colsum).
`nt_path()`, `split_path()` and `tn_path()` below mirror those rules; `test_gemm_dispatch_table_matches_sources` re-reads the thresholds and
the launcher conditions from the sources and checks that the cases of this file still reach every row, on the GPU and on the emulator.
Thresholds: OD_GEMM_SMALL_TILES 512 (emulator 6), OD_GEMM_QUARTER_TILES_F32 600 (emulator 6), OD_GEMM_BIG_MIN_M 32768 (emulator 256),
od_num_cus() 256 (emulator 16).  tn = ceil(N / 128), T = operand type (bf16, fp32, x3 = fp32 as 3 x bf16, x3w = x3 with a pre-split weight).

  row                                kernel                                  tile       selected when                                    e.g. GPU (M, N, K)
  w4/{none,silu}                     gemm_nt_w4_kernel<EPI> (persistent)     256 x 256  bf16, M >= BIG_MIN_M, N >= 256, N % 8 = 0,       32768 x 256 x 128
                                                                                        K % 128 = 0, no accumulate; grid min(tiles, CUs)
  w4/qkrope                          gemm_nt_w4_kernel<QKROPE>, in place                the same, q/k epilogue, hd 64                    33001 x 1536 x 128
  w4/qkrope-split{,-f16}             gemm_nt_w4_kernel<QKROPE>, qk_out                  od_gemm_nt_qkrope_split, the same (f16: half q/k/v) 33000 x 1536 x 256
  big/{bf16,fp32,x3,x3w}/{none,silu} gemm_nt_big_kernel<T, EPI> (8 waves)    256 x 256  M >= BIG_MIN_M, N >= 256, N % 8 = 0, K % BK = 0;  40000 x 520 x 192
                                                                                        bf16 only when K % 128 = 64
  big/bf16/accumulate                gemm_nt_big_kernel<bf16, NONE | SILU>   256 x 256  bf16 with accumulate (the w4 kernel refuses it)  33001 x 264 x 128
  big/bf16/{qkrope,qkrope-split}     gemm_nt_big_kernel<bf16, QKROPE>        256 x 256  q/k epilogue (hd 64), K % 128 = 64               33000 x 768 x 192
  nt/T/w{1,2,4}/{dma,reg}/EPI        gemm_nt_kernel<T, EPI, DMA, WMT>        32 WMT x 128 everything else: WMT 1 (fp32 only) when             4460 x 1408 x 512
                                                                                        ceil(M / 64) tn < QUARTER; WMT 2 when
                                                                                        ceil(M / 128) tn < SMALL; else WMT 4.
                                                                                        dma: K % BK = 0 (BK 64 bf16, 32 4-byte types),
                                                                                        3 LDS stages at WMT <= 2 except fp32, else 2.
                                                                                        EPI none / silu / qkrope (in place).  x3w has no
                                                                                        reg form: od_gemm_nt refuses K % 32 != 0.
  split-fallback/{bf16,fp32,x3}      od_gemm_nt, then od_qk_norm_rope        (as nt)    od_gemm_nt_qkrope_split outside the big/w4 rule  260 x 192 x 64
  tn_w4/bf16                         gemm_tn_w4_kernel                       256 x 256  bf16, M >= BIG_MIN_M, N, K >= 256, >= 8 256-tiles 33001 x 1365 x 512
                                                                                        (emulator: any tile count)
  tn/{bf16,fp32}/{2048,512}          gemm_tn_kernel<T>, ~2048 / 512 WGs      128 x 128  otherwise; 512 when <= 8 128-tiles and M >=      65536 x 512 x 256
                                                                                        BIG_MIN_M
  colsum/{bf16,fp32}                 colsum_kernel<T>                        256 cols   od_colsum                                        40000 x 1365

Every case runs with the deterministic shadow off; the TN and colsum cases also with it on (det.force(True)): same bound, and two runs bit-identical.

Memory contract: every output sits inside a wider NaN-prefilled buffer (non-zero column offset, ldc > N, rows past M), every operand inside
a NaN-poisoned one (columns K..lda of A and W, rows past M and N).  Afterwards every element outside the output is still NaN and none
inside is.  A kernel that reads outside its operand — or masks such a read by multiplying it with zero — fails, and so does one that writes
outside [M, N] or leaves an element unwritten.  A second layout (`NT.layout = "model"`, `TN.ldg` / `TN.lda`; tests/test_gemm_narrow_paths.py
runs it) is what LatentModel passes: contiguous operands and output, lda = ldw = K and ldc = N exactly (TN: chosen leading dimensions, NaN in
columns N..ldg and K..lda), each with 64 NaN elements either side.

Input families (built in fp32, rounded to the operand type; the reference reads the rounded operands back):
  integer       small integers (+-1, sparse enough that |C| <= 256): every product and sum is exact in fp32 and in bf16, so every path without
                the q/k epilogue must match fp64 bit for bit — a dropped or doubled slab, row or tile shows with zero tolerance.
  random        N(0, 1) (weights 0.3).
  range         row scales of A and of W spanning 2^-20 .. 2^20; compared after dividing both by the scale pair, so a tile that is wrong only
                at small magnitude counts as much as any other.
  cancel        rows of A and rows of W from complementary subspaces, plus 1e-3 noise: C is ~1e-3 of |A| |W|.  Measured against |A| |W|.
  lo_matters    (x3, x3w) positive fp32 operands whose bf16 low halves (2^-9 relative, all of one sign) carry the result: bf16 alone is off by
                ~2^-8 of |A| |W|, a dropped cross term by ~2^-9; x3 must reach 2^-15.
  silu_extreme  pre-activations of +-30 .. +-1e4 (through the bias): no NaN, the right sign, and zero where the true value underflows.
"""
import math
import os
import re
from dataclasses import dataclass

import pytest
import torch

from osu_dreamer_amd import _lib, det, ops
from kernel_backend import REPO, dev, tile_rel_l2  # noqa: F401

CSRC = os.path.join(REPO, "osu_dreamer_amd", "csrc")
NAN = float("nan")


@dataclass(frozen=True)
class Th:
    small: int        # OD_GEMM_SMALL_TILES
    quarter: int      # OD_GEMM_QUARTER_TILES_F32
    big_m: int        # OD_GEMM_BIG_MIN_M
    cus: int          # od_num_cus()


GPU_TH = Th(512, 600, 32768, 256)           # gemm.hip defaults, MI355X: checked against the sources below
EMU_TH = Th(6, 6, 256, 16)                  # tests/emu/build_emu.sh, od_api_internal.h
TN_BIG_MIN_TILES = 8
BK = {"bf16": 64, "fp32": 32, "x3": 32, "x3w": 32}      # elements per 128-byte k slab


def cdiv(a, b):
    return (a + b - 1) // b


@dataclass(frozen=True)
class Path:
    row: str
    kernel: str
    T: str
    tile: tuple               # (rows, columns) of the kernel's output tile
    wmt: int = 0
    dma: bool = True
    stages: int = 2
    grid: str = ""            # w4: "persistent" (more tiles than workgroups) or "one-round"


def nt_path(T, M, N, K, epi="none", acc=False, ldc=None, hd=64, n_rope=0, qk_out=False, th=GPU_TH):
    """The kernel launch_nt picks (see the table above).  epi: none, silu, qkrope (in place), qkrope-split, qkrope-split-f16."""
    ldc = N if ldc is None else ldc
    tiles_n = cdiv(N, 128)
    half = cdiv(M, 128) * tiles_n < th.small
    quarter = T == "fp32" and cdiv(M, 64) * tiles_n < th.quarter
    dma = K % BK[T] == 0
    rope = epi.startswith("qkrope")
    big_rope = rope and T == "bf16" and hd == 64 and n_rope % 64 == 0 and N % 64 == 0
    if (not rope or big_rope) and dma and M >= th.big_m and N % 8 == 0 and ldc % 8 == 0 and N >= 256:
        if T == "bf16" and not acc and K % 128 == 0:
            grid2 = cdiv(cdiv(M, 256), 8) * 8 * cdiv(N, 256)
            pgrid = max(8, th.cus & ~7)
            return Path(f"w4/{epi}", "gemm_nt_w4_kernel", T, (256, 256), grid="persistent" if grid2 > pgrid else "one-round")
        assert not epi.endswith("f16"), "the half q/k output exists in the w4 kernel only"
        if T == "bf16" and acc:
            return Path("big/bf16/accumulate", "gemm_nt_big_kernel", T, (256, 256))
        return Path(f"big/{T}/{epi}", "gemm_nt_big_kernel", T, (256, 256))
    assert not (rope and qk_out), "launch_nt refuses the split form outside the 256 x 256 kernels"
    wmt = (1 if T == "fp32" else 2) if quarter else 2 if half else 4
    stages = 3 if dma and wmt <= 2 and T != "fp32" else 2
    return Path(f"nt/{T}/w{wmt}/{'dma' if dma else 'reg'}/{epi}", "gemm_nt_kernel", T, (32 * wmt, 128), wmt, dma, stages)


def split_path(T, M, N, K, hd, n_rope, f16=False, th=GPU_TH):
    """od_gemm_nt_qkrope_split: one fused launch where the 256 x 256 kernels' epilogue applies, else od_gemm_nt + od_qk_norm_rope."""
    if T == "bf16" and hd == 64 and M >= th.big_m and K % 64 == 0 and N % 64 == 0 and N >= 256 and (not f16 or K % 128 == 0):
        return nt_path(T, M, N, K, "qkrope-split-f16" if f16 else "qkrope-split", hd=hd, n_rope=n_rope, qk_out=True, th=th)
    inner = nt_path(T, M, N, K, th=th)
    return Path(f"split-fallback/{'x3' if T == 'x3w' else T}", inner.kernel + " + od_qk_norm_rope", T, inner.tile, inner.wmt, inner.dma)


def tn_path(T, M, N, K, th=GPU_TH):
    if T == "bf16":
        tiles2 = cdiv(N, 256) * cdiv(K, 256)
        if M >= th.big_m and N >= 256 and K >= 256 and (tiles2 >= TN_BIG_MIN_TILES or th.big_m < 32768):
            return Path("tn_w4/bf16", "gemm_tn_w4_kernel", T, (256, 256))
    tiles = cdiv(N, 128) * cdiv(K, 128)
    target = 512 if tiles <= 8 and M >= th.big_m else 2048
    return Path(f"tn/{T}/{target}", "gemm_tn_kernel", T, (128, 128))


NT_ROWS = [f"nt/{T}/w{w}/{s}/{e}" for T in ("bf16", "x3", "x3w") for w in (2, 4) for s in ("dma", "reg") for e in ("none", "silu", "qkrope")
           if not (T == "x3w" and s == "reg")]
NT_ROWS += [f"nt/fp32/w{w}/{s}/{e}" for w in (1, 2, 4) for s in ("dma", "reg") for e in ("none", "silu", "qkrope")]
BIG_ROWS = [f"big/{T}/{e}" for T in ("bf16", "fp32", "x3", "x3w") for e in ("none", "silu")]
BIG_ROWS += ["big/bf16/accumulate", "big/bf16/qkrope", "big/bf16/qkrope-split"]
W4_ROWS = [f"w4/{e}" for e in ("none", "silu", "qkrope", "qkrope-split", "qkrope-split-f16")]
SPLIT_ROWS = [f"split-fallback/{T}" for T in ("bf16", "fp32", "x3")]
TN_ROWS = ["tn_w4/bf16", "tn/bf16/2048", "tn/bf16/512", "tn/fp32/2048", "tn/fp32/512"]
COLSUM_ROWS = ["colsum/bf16", "colsum/fp32"]
ROWS = NT_ROWS + BIG_ROWS + W4_ROWS + SPLIT_ROWS + TN_ROWS + COLSUM_ROWS
# rows the emulator's cases cannot reach: none — its thresholds (above) put every kernel of the table within reach of small shapes.  The
# GPU-only part of the coverage is the GPU thresholds' edges themselves, asserted separately (32767 / 32768 rows, 511 / 512 and 599 / 600
# tiles, a w4 grid of more workgroups than the chip's 256 CUs).
GPU_ONLY_ROWS = []

# ---------------------------------------------------------------- bounds
# Per output tile and over everything: relative L2 of (kernel - fp64 reference of the rounded operands).
#   output rounding: bf16 keeps 8 significant bits, so every element is within 2^-8 of its value and a tile within 2^-8 in relative L2 —
#     a hard bound, whatever the tile holds (the typical value is ~2^-9.5); fp32 / x3 outputs: 2^-24.
#   fp32 accumulation of K terms (the MFMA chain, in k order): one rounding of the running sum per term, each <= 2^-24 of |partial sum|
#     <= the row's |A| |W|; as a random walk sqrt(K) 2^-24 of it.  Against |C| of the random family (~ |A| |W| / sqrt(K) for the
#     incoherent sums) that is ~K 2^-24 / sqrt(K) = sqrt(K) 2^-24: ACC(K) below allows 4 sqrt(K) 2^-24 + 2^-22.
#   x3: a x b ~ hi hi + hi lo + lo hi drops lo lo (<= 2^-16 |a b|) and the rounding of each low half (<= 2^-17 |a|): <= 2^-15 of a
#     product, incoherent over k for the random family (~2^-15 / sqrt(3) of |C|), coherent for lo_matters (measured against |A| |W|).
# The previous suite compared one global rel-L2 of 2e-2 (bf16) — five times the bf16 bound here — and 2e-5 (fp32, x3).
U = {"bf16": 2.0 ** -8, "fp32": 2.0 ** -24, "x3": 2.0 ** -24, "x3w": 2.0 ** -24, "f16": 2.0 ** -11}


def ACC(K):
    return 4 * math.sqrt(K) * 2.0 ** -24 + 2.0 ** -22


def nt_bound(T, K, out="bf16", silu=False):
    u = U[out if T == "bf16" else out if out == "f16" else T]
    prod = 2.0 ** -15 if T in ("x3", "x3w") else 0.0
    b = u + ACC(K) + prod + (2.0 ** -19 if silu else 0.0)
    return (b, b)
# SiLU: x / (1 + exp(-x)) with the hardware exp (v_exp_f32 of -x log2 e) off by ~|x| 2^-24 relative: 2^-19 for the |x| <= 30 of these
# families (the extremes are checked element by element: check_silu_extreme).
# q/k epilogue: the pre-norm value is rounded to the tensor type (bf16: 2^-8) before the norm, the reference rounds the exact product the
# same way — they differ only where the fp32 sum sits within ACC(K) of a rounding midpoint, an ulp of one element now and then, which the
# norm carries to its head (~2^-8 / 8 relative per flip) — and the result is rounded once more: 2 x 2^-8 per tile.  fp32 / x3: the norm's
# 64-term sum of squares and rsqrt add a few 2^-24; x3's products as above.


def qk_bound(T, K, out):
    if out in ("bf16", "f16"):
        b = 2 * U[out] + ACC(K)
    else:
        b = 16 * 2.0 ** -24 + ACC(K) + (2.0 ** -15 if T in ("x3", "x3w") else 0.0)
    return (b, b)
# TN (dW, fp32 output) and colsum: fp32 sums of M products (bf16 x bf16 is exact in fp32; fp32 x fp32 rounds once, 2^-24) in M-split partial
# sums combined by atomics: ~sqrt(M) 2^-24 of |G|^T |A| for the random walk, which against |dW| of random operands is ~sqrt(M) 2^-24 again.


def tn_bound(M):
    b = 4 * math.sqrt(M) * 2.0 ** -24 + 2.0 ** -20
    return (b, b)


# ---------------------------------------------------------------- operands
TORCH = {"bf16": torch.bfloat16, "fp32": torch.float32, "x3": torch.float32, "x3w": torch.float32}


def _gen(device, seed):
    return torch.Generator(device=device).manual_seed(seed)


def integer_matrix(rows, cols, K, g, device, bound=16.0):
    """+-1 with density p so that a K-term sum has standard deviation `bound` (|sum| <= 256 by a wide margin)."""
    p = min(1.0, bound / math.sqrt(K))
    v = torch.randint(0, 2, (rows, cols), generator=g, device=device).float() * 2 - 1
    return v * (torch.rand(rows, cols, generator=g, device=device) < p)


def make_nt_inputs(fam, M, N, K, device, bias=True, acc=False, seed=0):
    """fp32 A (M, K), W (N, K), bias (N) or None, C0 (M, N) or None, and (range) the row scales of A and W."""
    g = _gen(device, seed)
    rn = lambda *s: torch.randn(*s, generator=g, device=device)         # noqa: E731
    ra = rw = None
    b = rn(N) if bias else None
    c0 = rn(M, N) if acc else None
    if fam == "integer":
        A, W = integer_matrix(M, K, K, g, device, 8.0), integer_matrix(N, K, K, g, device, 8.0)
        if bias:
            b = torch.randint(-4, 5, (N,), generator=g, device=device).float()
        if acc:
            c0 = torch.randint(-4, 5, (M, N), generator=g, device=device).float()
    elif fam == "random":
        A, W = rn(M, K), 0.3 * rn(N, K)
    elif fam == "range":
        ra = 2.0 ** torch.randint(-20, 21, (M,), generator=g, device=device).float()
        rw = 2.0 ** torch.randint(-20, 21, (N,), generator=g, device=device).float()
        A, W = rn(M, K) * ra[:, None], rn(N, K) * rw[:, None]
        b = c0 = None
    elif fam == "cancel":
        Q, _ = torch.linalg.qr(torch.randn(K, K, generator=g, device=device, dtype=torch.float64))
        h = K // 2
        A = (rn(M, h).double() @ Q[:, :h].t()).float() + 1e-3 * rn(M, K)
        W = (rn(N, K - h).double() @ Q[:, h:].t()).float() + 1e-3 * rn(N, K)
        b, c0 = None, 1e-3 * c0 if acc else None          # accumulate: onto values of C's own size
    elif fam == "lo_matters":
        def lo(rows):
            u = 1 + torch.randint(0, 128, (rows, K), generator=g, device=device).float() / 128      # bf16-exact, [1, 2)
            r = 0.2 + 0.7 * torch.rand(rows, K, generator=g, device=device)
            sgn = torch.randint(0, 2, (rows, 1), generator=g, device=device).float() * 2 - 1
            return sgn * u * (1 + 2.0 ** -9 * r)                                                   # bf16(x) = u: the low half is u r 2^-9
        A, W = lo(M), lo(N)
        b = c0 = None
    elif fam == "silu_extreme":
        A, W = 0.05 * rn(M, K), 0.05 * rn(N, K) / math.sqrt(K)
        mag = 30.0 * (1e4 / 30.0) ** torch.rand(N, generator=g, device=device)
        sgn = torch.randint(0, 2, (N,), generator=g, device=device).float() * 2 - 1
        b = sgn * mag
    else:
        raise AssertionError(fam)
    return A, W, b, c0, ra, rw


def poisoned(t, rows, cols, r0=0, c0=0, dtype=None):
    """A NaN buffer of (rows, cols) holding `t` at (r0, c0); returns (buffer, view)."""
    buf = torch.full((rows, cols), NAN, dtype=dtype or t.dtype, device=t.device)
    v = buf[r0:r0 + t.shape[0], c0:c0 + t.shape[1]]
    v.copy_(t)
    return buf, v


def assert_contract(case, buf, r0, c0, M, N, what="C"):
    inside = torch.zeros(buf.shape, dtype=torch.bool, device=buf.device)
    inside[r0:r0 + M, c0:c0 + N] = True
    nan = torch.isnan(buf.float())
    bad_out = int((~nan & ~inside).sum())
    assert bad_out == 0, f"{case}: {bad_out} elements outside {what}[{M}, {N}] were written"
    bad_in = nan[r0:r0 + M, c0:c0 + N]
    if bool(bad_in.any()):
        r, c = (int(i) for i in bad_in.nonzero()[0])
        raise AssertionError(f"{case}: {int(bad_in.sum())} elements of {what} are NaN (unwritten, or read from the poisoned padding), first "
                             f"({r}, {c})")


def bits(t):
    return t.view(torch.int16 if t.element_size() == 2 else torch.int32)


def flat_buffer(shape, dtype, device, fill=None):
    """The `model` layout: a contiguous tensor of `shape` (NaN, or a copy of `fill`) with 64 NaN elements either side; returns (buffer, view)."""
    n = math.prod(shape)
    buf = torch.full((n + 128,), NAN, dtype=dtype, device=device)
    v = buf[64:64 + n].view(*shape)
    if fill is not None:
        v.copy_(fill)
    return buf, v


def assert_flat_contract(case, buf, what="C"):
    nan = torch.isnan(buf.float())
    n = buf.numel() - 128
    bad_out = int((~nan[:64]).sum() + (~nan[64 + n:]).sum())
    assert bad_out == 0, f"{case}: {bad_out} elements outside the contiguous {what} were written"
    assert not bool(nan[64:64 + n].any()), f"{case}: {int(nan[64:64 + n].sum())} elements of {what} are NaN (unwritten, or read from the poisoned " \
                                           f"padding), first at flat index {int(nan[64:64 + n].nonzero()[0])}"


# ---------------------------------------------------------------- NT cases
@dataclass
class NT:
    T: str
    M: int
    N: int
    K: int
    epi: str = "none"        # none, silu, qkrope, qkrope-split, qkrope-split-f16
    fam: str = "random"
    acc: bool = False
    bias: bool = True
    hd: int = 64
    L: int = 0               # q/k epilogue: rows per sequence (table positions row % L); 0: M
    seed: int = 0
    layout: str = "fenced"   # fenced: operands and output inside wider NaN buffers (below); model: contiguous, lda = ldw = K and ldc = N,
                             # 64 NaN elements either side of each (what LatentModel passes; epilogues none and silu)

    @property
    def n_rope(self):
        return 2 * (self.N // 3) if self.epi.startswith("qkrope") else 0

    @property
    def id(self):
        ex = ("-acc" if self.acc else "") + ("" if self.bias else "-nobias") + (f"-hd{self.hd}" if self.n_rope else "")
        ex += "" if self.layout == "fenced" else "-" + self.layout
        return f"{self.T}-{self.epi}-{self.fam}{ex}-{self.M}x{self.N}x{self.K}"

    @property
    def ldc(self):
        return ldc_of(self.N) if self.layout == "fenced" else self.N

    def path(self, th=GPU_TH):
        if self.epi.startswith("qkrope-split"):
            return split_path(self.T, self.M, self.N, self.K, self.hd, self.n_rope, self.epi.endswith("f16"), th)
        return nt_path(self.T, self.M, self.N, self.K, self.epi, self.acc, self.ldc, self.hd, self.n_rope, th=th)


def ldc_of(N):
    return cdiv(N + 8 + 24, 8) * 8            # output column offset 8, >= 24 NaN columns behind it, a multiple of 8


def run_nt(c: NT, device, twice=False):
    T, M, N, K = c.T, c.M, c.N, c.K
    tt = TORCH[T]
    out_t = "bf16" if T == "bf16" else "fp32"
    A32, W32, b, c0, ra, rw = make_nt_inputs(c.fam, M, N, K, device, c.bias and c.fam not in ("range", "cancel", "lo_matters"), c.acc, c.seed)
    model = c.layout == "model"
    assert c.layout in ("fenced", "model") and not (model and (T == "x3w" or c.n_rope))
    lda, ldw = cdiv(K + 8, 8) * 8 + 8, cdiv(K + 8, 8) * 8 + 16
    _, A = flat_buffer((M, K), tt, device, A32.to(tt)) if model else poisoned(A32.to(tt), M + 5, lda)
    if model:
        _, W = flat_buffer((N, K), tt, device, W32.to(tt))
        Wr = W
    elif T == "x3w":
        st = torch.zeros(N + 3, cdiv(K, 32) * 32 + 32, device=device)
        ops.pack_weight(W32, ops.SplitWeight(st))                    # per 32-element k slab: 32 bf16 high halves, then 32 low halves
        st[N:, :] = NAN
        st[:, K:] = NAN                 # whole slabs past K
        W = ops.SplitWeight(st[:N, :K])
        Wr = W32
    else:
        _, W = poisoned(W32.to(tt), N + 7, ldw)
        Wr = W
    x3 = T in ("x3", "x3w")
    Ad, Wd = A.double(), Wr.double()
    if c0 is not None:
        c0 = c0.to(tt)
    prod = Ad @ Wd.t()
    bd = b.double() if b is not None else None

    def launch():
        if model:
            buf, C = flat_buffer((M, N), tt, device, c0)
        else:
            buf = torch.full((M + 3, c.ldc), NAN, dtype=tt, device=device)
            C = buf[:M, 8:8 + N]
            if c0 is not None:
                C.copy_(c0)
        if c.epi in ("none", "silu"):
            ops.gemm_nt(A, W, b, C, epilogue=ops.OD_EPI_SILU if c.epi == "silu" else ops.OD_EPI_NONE, accumulate=c.acc, x3=x3)
            return buf, C, None, None
        H, hd, L = c.n_rope // (2 * c.hd), c.hd, c.L or M
        if c.epi == "qkrope":
            ops.gemm_nt_qkrope(A, W, b, C, wq, wk, tab, L, H, hd, EPS, x3=x3, q_scale=QS)
            return buf, C, None, None
        f16 = c.epi.endswith("f16")
        qbuf = torch.full((M + 2, c.n_rope + 24), NAN, dtype=torch.float16 if f16 else tt, device=device)
        qk = qbuf[:M, 8:8 + c.n_rope]
        ops.gemm_nt_qkrope_split(A, W, b, C, qk, wq, wk, tab, L, H, hd, EPS, x3=x3, q_scale=QS)
        return buf, C, qbuf, qk

    if c.n_rope:
        g = _gen(device, 100 + c.seed)
        wq = 1 + 0.2 * torch.randn(c.hd, generator=g, device=device)
        wk = 1 + 0.2 * torch.randn(c.hd, generator=g, device=device)
        L = c.L or M
        tab = torch.zeros(L, c.hd // 2, 2, device=device)
        ops.rope_table(tab, L, c.hd)
    buf, C, qbuf, qk = launch()
    p = c.path(GPU_TH if device.type == "cuda" else EMU_TH)        # the backend's own thresholds: its kernel's tile, its row in the label
    case = f"{c.id} [{p.row}]"
    if model:
        assert_flat_contract(case, buf)
    else:
        assert_contract(case, buf, 0, 8, M, N)
    tr, tc = p.tile
    pre = prod + bd if bd is not None else prod

    if c.epi.startswith("qkrope"):
        f16 = c.epi.endswith("f16")
        nr = c.n_rope
        # the pre-norm values as the kernel rounds them: bf16 / fp32 — the half form's q / k norm reads the same bf16 values
        pre_r = pre.to(tt).double()
        ref_qk = qk_reference(pre_r, tab.double(), wq.double(), wk.double(), c.L or M, nr // (2 * c.hd), c.hd)
        fallback = p.row.startswith("split-fallback")
        if qk is None:                                   # in place: q / k normed + rotated in C, v as the product
            check_tiles(case, "q/k", C[:, :nr], ref_qk, tr, min(tc, nr), qk_bound(T, K, out_t))
            check_tiles(case, "v", C[:, nr:], pre[:, nr:], tr, tc, nt_bound(T, K, out_t))
        else:                                            # split: q / k to qk_out, C keeps the pre-norm product (v in half with f16)
            assert_contract(case, qbuf, 0, 8, M, nr, "qk_out")
            check_tiles(case, "q/k", qk, ref_qk, tr, min(tc, nr), qk_bound(T, K, "f16" if f16 else out_t))
            check_tiles(case, "pre-norm q/k", C[:, :nr], pre[:, :nr], tr, min(tc, nr), nt_bound(T, K, out_t))
            v = C[:, nr:].view(torch.float16) if f16 else C[:, nr:]
            # the half v of the two-kernel form is the bf16 product re-encoded (bf16 rounding); the w4 kernel rounds fp32 to half once
            check_tiles(case, "v", v, pre[:, nr:], tr, tc, nt_bound(T, K, "f16" if f16 and not fallback else out_t))
        if twice:
            buf2, C2, qbuf2, _ = launch()
            assert torch.equal(bits(buf2), bits(buf)) and (qbuf is None or torch.equal(bits(qbuf2), bits(qbuf))), f"{case}: two runs differ"
        return

    ref = pre
    if c.epi == "silu":
        ref = ref * torch.sigmoid(ref)
    if c0 is not None:
        ref = ref + c0.double()
    out = C.double()
    if c.fam == "integer":
        assert float(ref.abs().max()) <= 256, "the integer fixture must keep |C| exact in bf16"
        if c.epi == "none":
            bad = out != ref
            if bool(bad.any()):
                r, col = (int(i) for i in bad.nonzero()[0])
                raise AssertionError(f"{case}: {int(bad.sum())} elements differ from the exact product, first ({r}, {col}) = {float(out[r, col])}"
                                     f" against {float(ref[r, col])}, tile {(r // tr, col // tc)}")
            measured(case, "C (exact)", out, 0.0, 0.0)
        else:
            check_tiles(case, "C", out, ref, tr, tc, nt_bound(T, K, out_t, silu=True))
    elif c.fam == "silu_extreme":
        check_silu_extreme(case, out, ref, out_t)
    elif c.fam == "range":
        s = ra.double()[:, None] * rw.double()[None, :]
        check_tiles(case, "C / (scale_a scale_w)", out / s, ref / s, tr, tc, nt_bound(T, K, out_t))
    elif c.fam in ("cancel", "lo_matters"):
        sc = Ad.abs() @ Wd.abs().t()
        check_tiles(case, "C against |A| |W|", out, ref, tr, tc, LO_BOUND if c.fam == "lo_matters" else nt_bound(T, K, out_t), scale=sc)
    else:
        check_tiles(case, "C", out, ref, tr, tc, nt_bound(T, K, out_t, silu=c.epi == "silu"))
    if twice:
        buf2, _, _, _ = launch()
        assert torch.equal(bits(buf2), bits(buf)), f"{case}: two runs into fresh buffers differ"


EPS, QS = 1.2e-7, 0.18
LO_BOUND = (2.0 ** -15, 2.0 ** -15)      # x3 / x3w on lo_matters, against |A| |W|: the dropped lo lo and low-half roundings (bf16 alone: ~2^-8)


def qk_reference(pre, tab, wq, wk, L, H, hd):
    """head_rms_norm + rope_half_split (oracle/denoiser_oracle.py) in fp64 on the rounded pre-norm values, with the kernel's own (cos, sin)
    table (row m at position m % L), q scaled by QS."""
    M = pre.shape[0]
    dh, half = H * hd, hd // 2
    pos = torch.arange(M, device=pre.device) % L
    cs, sn = tab[pos, :, 0][:, None, :], tab[pos, :, 1][:, None, :]
    outs = []
    for part, w, s in ((pre[:, :dh], wq, QS), (pre[:, dh:2 * dh], wk, 1.0)):
        x = part.reshape(M, H, hd)
        y = x * torch.rsqrt(x.pow(2).mean(-1, keepdim=True) + EPS) * w * s
        a, b = y[..., :half], y[..., half:]
        outs.append(torch.cat([a * cs - b * sn, a * sn + b * cs], -1).reshape(M, dh))
    return torch.cat(outs, 1)


def measured(case, what, out, err, bound):
    """One line per check for the summaries of a run (pytest -s, or the captured output of a failure): `case` ends in its dispatch row."""
    print(f"MEASURED {case} {what} {'hip' if out.device.type == 'cuda' else 'emu'} {err:.3e} {bound:.3e}")


def check_tiles(case, what, out, ref, tr, tc, bound, scale=None):
    blk, glob, where = tile_rel_l2(out, ref, tr, tc, scale=scale)
    measured(case, what, out, blk, bound[0])
    assert blk <= bound[0] and glob <= bound[1], f"{case} {what}: tile {blk:.3e} at (tile row, tile column) {where} of {tr} x {tc}, global " \
                                                 f"{glob:.3e}, bounds ({bound[0]:.3e}, {bound[1]:.3e})"


def check_silu_extreme(case, out, ref, out_t):
    assert not bool(torch.isnan(out).any()), f"{case}: NaN from SiLU"
    tiny = ref.abs() < 1e-30
    # fp32: v_exp_f32 of x log2(e) is off by ~|x| 2^-24 relative; bf16 adds its output rounding
    rtol = (2.0 ** -8 if out_t == "bf16" else 0.0) + 1e-5
    big = ~tiny
    err = ((out - ref).abs() / ref.abs().clamp_min(1e-300))[big]
    assert float(err.max()) <= rtol, f"{case}: SiLU relative error {float(err.max()):.3e}"
    assert bool((torch.sign(out[big]) == torch.sign(ref[big])).all()), f"{case}: SiLU sign"
    assert bool((out[tiny].abs() <= 1e-30).all() & (out[tiny] <= 0).all()), f"{case}: SiLU of a large negative input must be (-)0"


# ---------------------------------------------------------------- the NT cases
# Emulator thresholds (small 6, quarter 6, big 256): the shapes below reach every gemm_nt_kernel instantiation with M % tile in {1, tile - 1}
# (65 / 127 at WMT 2, 129 / 383 (255 fp32) at WMT 4, 33 / 95 at WMT 1), N ragged against 128 (130, 136, 264) and N % 8 != 0 (130: the scalar epilogue).
SHAPES = {("bf16", 2): [(65, 136), (127, 264)], ("bf16", 4): [(129, 264), (383, 130)],
          ("fp32", 1): [(33, 136), (95, 130)], ("fp32", 2): [(129, 136), (255, 130)], ("fp32", 4): [(129, 264), (255, 264)]}
for _w in (2, 4):
    SHAPES[("x3", _w)] = SHAPES[("x3w", _w)] = SHAPES[("bf16", _w)]
QK_SHAPES = {2: [(65, 192), (127, 192)], 4: [(257, 192), (383, 192)]}
QK_SHAPES_F32 = {1: [(33, 192), (95, 192)], 2: [(129, 192), (255, 192)], 4: [(257, 192), (383, 192)]}


def slab_counts(T, wmt, dma):
    """K values: k-slab counts 1, 2, stages, stages + 1 (DMA), or K not a multiple of the slab (register staging)."""
    bk = BK[T]
    if not dma:
        return [bk + 8 if T == "bf16" else bk + 4, 3 * bk + 8 if T == "bf16" else 3 * bk + 4]
    stages = 3 if wmt <= 2 and T != "fp32" else 2
    return [bk * n for n in sorted({1, 2, stages, stages + 1})]


SMALL = []
for (T, wmt), shapes in SHAPES.items():
    for dma in (True, False):
        if T == "x3w" and not dma:
            continue
        Ks = slab_counts(T, wmt, dma)
        for i, K in enumerate(Ks):                                 # the exact family at every slab count, accumulate + bias on one
            SMALL.append(NT(T, *shapes[i % 2], K, "none", "integer", acc=i == 1, seed=i))
        SMALL.append(NT(T, *shapes[1], Ks[-1], "none", "random"))
        SMALL.append(NT(T, *shapes[0], Ks[-1], "none", "random", acc=True, bias=False))
        SMALL.append(NT(T, *shapes[0], Ks[0], "silu", "random", acc=True))
        SMALL.append(NT(T, *shapes[1], Ks[-1], "silu", "silu_extreme"))
        SMALL.append(NT(T, *shapes[1], Ks[0], "silu", "integer"))
        if dma:
            SMALL.append(NT(T, *shapes[0], Ks[-1], "none", "range"))
            SMALL.append(NT(T, *shapes[1], Ks[-1], "none", "cancel"))
        if T in ("x3", "x3w"):
            SMALL.append(NT(T, *shapes[1], Ks[-1], "none", "lo_matters"))
        qks = (QK_SHAPES_F32 if T == "fp32" else QK_SHAPES)[wmt]
        for j, (M, N) in enumerate(qks):
            SMALL.append(NT(T, M, N, Ks[-1 if j else 0], "qkrope", "random", hd=64 if j else 32, L=M // 2 + 1))
# the 256 x 256 kernels on the emulator (M >= 256): w4 with one round of tiles (300 x 264: 8 tiles < 16 "CUs") and several (2100 x 264:
# 32 > 16 tiles, ragged last row tile), the 8-wave kernel for the other types, bf16 accumulate and bf16 K % 128 = 64
SMALL += [NT("bf16", 300, 264, 128, "none", "integer"), NT("bf16", 2100, 264, 128, "none", "integer"), NT("bf16", 1300, 520, 256, "none", "random"),
          NT("bf16", 257, 264, 256, "none", "range", seed=1), NT("bf16", 300, 264, 128, "silu", "random"), NT("bf16", 511, 264, 128, "silu", "silu_extreme"),
          NT("bf16", 300, 264, 192, "none", "integer"), NT("bf16", 257, 264, 64, "none", "random"), NT("bf16", 300, 264, 192, "silu", "random"),
          NT("bf16", 300, 264, 128, "none", "integer", acc=True), NT("bf16", 257, 264, 192, "silu", "random", acc=True),
          NT("bf16", 300, 264, 64, "none", "random", acc=True, bias=False)]
for T, Ks in (("fp32", (32, 96)), ("x3", (64, 96)), ("x3w", (32, 128))):
    SMALL += [NT(T, 257, 264, Ks[0], "none", "integer"), NT(T, 300, 264, Ks[1], "none", "random", acc=True), NT(T, 511, 264, Ks[1], "silu", "random"),
              NT(T, 300, 264, Ks[0], "none", "cancel")]
    if T != "fp32":
        SMALL.append(NT(T, 300, 264, Ks[1], "none", "lo_matters"))
# q/k epilogue in the 256 x 256 kernels (bf16, hd 64, N = 3 x 128): w4 at K % 128 = 0, the 8-wave kernel at K % 128 = 64; split forms need M % L = 0;
# the two-kernel fallback of the split form for every type
SMALL += [NT("bf16", 260, 384, 128, "qkrope", L=70), NT("bf16", 260, 384, 192, "qkrope", L=70), NT("bf16", 260, 384, 256, "qkrope-split", L=130),
          NT("bf16", 260, 384, 128, "qkrope-split-f16", L=130), NT("bf16", 390, 384, 64, "qkrope-split", L=130),
          NT("bf16", 130, 192, 64, "qkrope-split", L=65), NT("fp32", 130, 192, 96, "qkrope-split", L=65), NT("x3", 130, 192, 96, "qkrope-split", L=65),
          NT("x3w", 130, 192, 64, "qkrope-split", L=65), NT("x3", 260, 384, 100, "qkrope-split", hd=32, L=130)]

# GPU sizes (GPU thresholds): WMT 4 of the 128-row kernel needs >= 512 128-row tiles, fp32 WMT 2 >= 600 64-row tiles, the 256 x 256 kernels
# >= 32768 rows.  The edges: 3969 x 2048 is 512 tiles, 9343 x 832 is 511; 38336 x 128 is 599 64-row tiles (fp32 WMT 1), 38337 x 128 600;
# M 32767 / 32768; the sampler (4460 rows) and the batched sampler (G = 8: 49152 rows); w4 grids of 128 and 1120 workgroups; N >= 1024
# (non-temporal stores).
GPU_CASES = [
    NT("bf16", 3969, 2048, 192, "none", "integer"), NT("bf16", 3969, 2048, 192, "none", "random", acc=True), NT("bf16", 3969, 2048, 200, "none", "integer"),
    NT("bf16", 3969, 2048, 200, "silu", "random"), NT("bf16", 3969, 2048, 64, "silu", "silu_extreme"), NT("bf16", 9343, 832, 256, "none", "integer"),
    NT("bf16", 9343, 832, 72, "none", "random"), NT("bf16", 32767, 264, 128, "none", "integer"), NT("bf16", 32767, 264, 128, "none", "range"),
    NT("bf16", 5377, 1536, 128, "qkrope", L=1115), NT("bf16", 5377, 1536, 200, "qkrope", L=1115),
    NT("x3", 3969, 2048, 96, "none", "integer"), NT("x3", 3969, 2048, 96, "none", "lo_matters"), NT("x3", 3969, 2048, 100, "none", "random"),
    NT("x3", 3969, 2048, 100, "silu", "random"), NT("x3", 3969, 2048, 32, "silu", "random"), NT("x3", 4460, 1408, 512, "none", "random"),
    NT("x3", 5377, 1536, 96, "qkrope", L=1115), NT("x3", 5377, 1536, 100, "qkrope", L=1115),
    NT("x3w", 3969, 2048, 128, "none", "integer"), NT("x3w", 3969, 2048, 128, "none", "lo_matters"), NT("x3w", 3969, 2048, 64, "silu", "random"),
    NT("x3w", 4460, 3072, 512, "none", "random"), NT("x3w", 5377, 1536, 96, "qkrope", L=1115),
    NT("fp32", 38336, 128, 64, "none", "integer"), NT("fp32", 38337, 128, 64, "none", "integer"), NT("fp32", 4460, 1408, 512, "none", "random"),
    NT("fp32", 4460, 1408, 100, "none", "random", acc=True), NT("fp32", 4460, 1408, 96, "silu", "random"), NT("fp32", 4460, 1408, 100, "silu", "random"),
    NT("fp32", 3969, 2048, 96, "none", "integer"), NT("fp32", 3969, 2048, 100, "none", "range"), NT("fp32", 3969, 2048, 96, "silu", "silu_extreme"),
    NT("fp32", 3969, 2048, 36, "silu", "random"),
    NT("fp32", 4460, 1536, 256, "qkrope", L=1115), NT("fp32", 4460, 1536, 100, "qkrope", L=1115), NT("fp32", 5377, 1536, 96, "qkrope", L=1115),
    NT("fp32", 5377, 1536, 100, "qkrope", L=1115),
    # the 256 x 256 kernels
    NT("bf16", 32768, 256, 128, "none", "integer"), NT("bf16", 70000, 1024, 256, "none", "random"), NT("bf16", 40000, 1408, 128, "silu", "random"),
    NT("bf16", 33001, 1408, 576, "none", "integer"), NT("bf16", 40000, 520, 64, "none", "random"), NT("bf16", 40000, 520, 192, "silu", "random"),
    NT("bf16", 33001, 264, 128, "none", "integer", acc=True), NT("bf16", 33001, 1024, 128, "silu", "random", acc=True),
    NT("fp32", 32768, 264, 96, "none", "integer"), NT("fp32", 40000, 1024, 32, "silu", "random"), NT("fp32", 33001, 520, 64, "none", "random", acc=True),
    NT("x3", 32768, 264, 96, "none", "integer"), NT("x3", 33001, 520, 64, "silu", "random"), NT("x3", 33001, 520, 96, "none", "lo_matters"),
    NT("x3w", 49152, 512, 512, "none", "random"), NT("x3w", 49152, 1536, 128, "silu", "random"), NT("x3w", 32768, 264, 64, "none", "lo_matters"),
    NT("bf16", 33001, 1536, 128, "qkrope", L=1115), NT("bf16", 33000, 1536, 256, "qkrope-split", L=8250),
    NT("bf16", 33000, 1536, 256, "qkrope-split-f16", L=8250), NT("bf16", 33000, 768, 192, "qkrope", L=8250),
    NT("bf16", 33000, 768, 192, "qkrope-split", L=8250), NT("fp32", 33000, 768, 192, "qkrope-split", L=8250),
    NT("x3", 33000, 768, 100, "qkrope-split", L=8250),
]


# ---------------------------------------------------------------- TN and colsum
@dataclass
class TN:
    T: str
    M: int
    N: int
    K: int
    fam: str = "random"
    det: bool = False
    blk: int = 0             # od_gemm_tn_blocks: columns of G in blocks of `blk`, the first `valid` live
    valid: int = 0
    bias: bool = True
    ldg: int = 0             # both 0: G and A as column sub-views of wider NaN buffers (below).  Otherwise the layout LatentModel passes:
    lda: int = 0             # contiguous G (M, ldg >= N) and A (M, lda >= K), NaN in columns N..ldg and K..lda, 64 NaN elements either side

    @property
    def id(self):
        ex = f"-ldg{self.ldg}-lda{self.lda}" if self.ldg else ""
        return f"{self.T}-{self.fam}{'-det' if self.det else ''}{f'-blk{self.blk}v{self.valid}' if self.blk else ''}{ex}-{self.M}x{self.N}x{self.K}"

    def path(self, th=GPU_TH):
        return tn_path(self.T, self.M, self.N, self.K, th)


def det_run(device, on, outs, fn):
    """fn() with the deterministic shadow on (outs registered, flushed afterwards) or off."""
    if not on:
        fn()
        return
    try:
        det.force(True)
        ctx = det.context(device)
        for t in outs:
            ctx.register(t)
        fn()
        for t in outs:
            ctx.flush(t)
    finally:
        det.force(None)


def run_tn(c: TN, device, twice=False):
    T, M, N, K = c.T, c.M, c.N, c.K
    tt = TORCH[T]
    g = _gen(device, 7)
    if c.fam == "integer":
        G32, A32 = integer_matrix(M, N, M, g, device, 64.0), integer_matrix(M, K, M, g, device, 64.0)
        dW0 = torch.randint(-8, 9, (N, K), generator=g, device=device).float()
    else:
        G32, A32 = torch.randn(M, N, generator=g, device=device), torch.randn(M, K, generator=g, device=device)
        dW0 = torch.randn(N, K, generator=g, device=device)
    if c.ldg or c.lda:
        assert c.ldg >= N and c.lda >= K
        _, Gf = flat_buffer((M, c.ldg), tt, device)
        _, Af = flat_buffer((M, c.lda), tt, device)
        G, A = Gf[:, :N], Af[:, :K]
        G.copy_(G32)
        A.copy_(A32)
    else:
        ldg, lda = cdiv(N, 8) * 8 + 24, cdiv(K, 8) * 8 + 16
        _, G = poisoned(G32.to(tt), M + 3, ldg, 0, 8)             # column sub-views of wider NaN buffers (16-byte aligned)
        _, A = poisoned(A32.to(tt), M + 5, lda, 0, 8)
    Gd, Ad = G.double(), A.double()
    if c.blk:
        live = torch.tensor([n for n in range(N) if n % c.blk < c.valid], device=device)
        rows = len(live)
    else:
        live, rows = torch.arange(N, device=device), N
    ref = dW0.double()[:rows] + Gd[:, live].t() @ Ad
    refb = 1.0 + Gd[:, live].sum(0)

    def launch():
        pad = 64
        flat = torch.full((2 * pad + rows * K,), NAN, device=device)
        dW = flat[pad:pad + rows * K].view(rows, K)
        dW.copy_(dW0[:rows])
        bflat = torch.full((2 * pad + rows,), NAN, device=device)
        db = bflat[pad:pad + rows]
        db.fill_(1.0)
        det_run(device, c.det, [dW, db] if c.bias else [dW],
                lambda: ops.gemm_tn(G, A, dW, n_cols=N, k_cols=K, dbias=db if c.bias else None, n_block=c.blk, n_valid=c.valid))
        return flat, dW, bflat, db

    flat, dW, bflat, db = launch()
    p = c.path(GPU_TH if device.type == "cuda" else EMU_TH)        # the backend's own thresholds: its kernel's tile, its row in the label
    case = f"{c.id} [{p.row}]"
    assert not bool(torch.isnan(dW).any()) and bool(torch.isnan(flat[:64]).all() & torch.isnan(flat[64 + rows * K:]).all()), f"{case}: dW contract"
    assert not bool(torch.isnan(db).any()) and bool(torch.isnan(bflat[:64]).all() & torch.isnan(bflat[64 + rows:]).all()), f"{case}: dbias contract"
    if not c.bias:
        refb = torch.ones_like(refb)
    if c.fam == "integer":
        assert float(ref.abs().max()) < 2 ** 24
        bad = dW.double() != ref
        assert not bool(bad.any()), f"{case}: {int(bad.sum())} elements of dW differ from the exact sum, first {tuple(int(i) for i in bad.nonzero()[0])}"
        assert torch.equal(db.double(), refb), f"{case}: dbias differs from the exact column sums"
        measured(case, "dW, dbias (exact)", dW, 0.0, 0.0)
    else:
        check_tiles(case, "dW", dW.double(), ref, *p.tile, tn_bound(M))
        check_tiles(case, "dbias", db.double()[None, :], refb[None, :], 1, p.tile[0], tn_bound(M))
    if twice or c.det:
        flat2, _, bflat2, _ = launch()
        if c.det or c.fam == "integer":
            assert torch.equal(bits(flat2), bits(flat)) and torch.equal(bits(bflat2), bits(bflat)), f"{case}: two runs differ"


def run_colsum(T, M, N, on, device):
    tt = TORCH[T]
    g = _gen(device, 9)
    _, G = poisoned(torch.randn(M, N, generator=g, device=device).to(tt), M + 2, cdiv(N, 8) * 8 + 24, 0, 8)
    ref = G.double().sum(0)

    def launch():
        flat = torch.full((N + 128,), NAN, device=device)
        out = flat[64:64 + N]
        out.fill_(0.5)
        det_run(device, on, [out], lambda: ops.colsum(G, out))
        return flat, out
    flat, out = launch()
    case = f"colsum-{T}{'-det' if on else ''}-{M}x{N}"
    assert bool(torch.isnan(flat[:64]).all() & torch.isnan(flat[64 + N:]).all()) and not bool(torch.isnan(out).any()), f"{case}: contract"
    check_tiles(case, "sum", out.double()[None, :] - 0.5, ref[None, :], 1, 256, tn_bound(M))
    if on:
        flat2, _ = launch()
        assert torch.equal(bits(flat2), bits(flat)), f"{case}: two deterministic runs differ"


TN_SMALL = [TN("bf16", 200, 136, 72, "integer"), TN("bf16", 200, 136, 72), TN("bf16", 600, 136, 200, "integer"), TN("bf16", 600, 130, 200),
            TN("bf16", 600, 264, 264, "integer"), TN("bf16", 700, 272, 264, blk=136, valid=130), TN("bf16", 300, 48, 40, "integer", blk=24, valid=17),
            TN("fp32", 200, 136, 72, "integer"), TN("fp32", 200, 130, 36), TN("fp32", 600, 130, 200, "integer"), TN("fp32", 600, 136, 200),
            TN("fp32", 300, 48, 40, blk=24, valid=17), TN("bf16", 200, 130, 72, bias=False)]
TN_SMALL += [TN(c.T, c.M, c.N, c.K, c.fam, True, c.blk, c.valid) for c in TN_SMALL[:12:2]] + [TN("bf16", 600, 264, 264, "random", True),
                                                                                              TN("fp32", 600, 130, 200, "random", True)]
TN_GPU = [TN("bf16", 33001, 1365, 512, "integer"), TN("bf16", 40000, 3072, 512), TN("bf16", 40000, 136, 512, "integer"), TN("bf16", 40000, 136, 512),
          TN("bf16", 20000, 264, 264), TN("fp32", 65536, 512, 256, "integer"), TN("fp32", 65536, 512, 256), TN("fp32", 50001, 512, 1365),
          TN("fp32", 50001, 1365, 512, "integer"), TN("bf16", 32768, 2816, 512, blk=1408, valid=1365)]
TN_GPU += [TN("bf16", 33001, 1365, 512, "random", True), TN("bf16", 40000, 136, 512, "random", True), TN("fp32", 65536, 512, 256, "random", True),
           TN("fp32", 50001, 512, 1365, "integer", True), TN("bf16", 20000, 264, 264, "integer", True)]
COLSUM_SMALL = [("bf16", 700, 130), ("fp32", 300, 1365)]
COLSUM_GPU = [("bf16", 40000, 1365), ("fp32", 50001, 512)]


# ---------------------------------------------------------------- dispatch table
def _emu_rows():
    rows = {c.path(EMU_TH).row for c in SMALL} | {c.path(EMU_TH).row for c in TN_SMALL}
    return rows | {f"colsum/{T}" for T, _, _ in COLSUM_SMALL}


def _gpu_rows():
    rows = {c.path(GPU_TH).row for c in SMALL + GPU_CASES} | {c.path(GPU_TH).row for c in TN_SMALL + TN_GPU}
    return rows | {f"colsum/{T}" for T, _, _ in COLSUM_SMALL + COLSUM_GPU}


# the GEMM shapes the rest of the suite runs on the emulator (tests/test_kernels.py): each still reaches a row of the table under the
# emulator's thresholds (the fp32 quarter-tile threshold was lowered there to 6 so fp32 WMT 2 / 4 run on the emulator too)
EXISTING_EMU = [(T, M, N, K) for T in ("bf16", "fp32") for M, N, K in ((200, 136, 96), (128, 128, 64), (77, 24, 16), (300, 384, 192), (2100, 520, 128),
                                                                       (1500, 264, 256))]
EXISTING_EMU += [("x3", M, N, K) for M, N, K in ((200, 136, 96), (300, 384, 192), (512, 512, 256))]
EXISTING_EMU += [("x3w", M, N, K) for M, N, K in ((200, 136, 96), (300, 384, 192), (512, 512, 256))]


def test_gemm_dispatch_table_matches_sources():
    """The thresholds and launcher conditions the path functions mirror are the ones in the sources; the cases of this file reach every
    row of the table on the GPU, and every row the emulator's thresholds allow on the emulator."""
    src = open(os.path.join(CSRC, "gemm.hip")).read()
    defs = {k: int(v) for k, v in re.findall(r"#define (OD_\w+) (\d+)", src)}
    assert (defs["OD_GEMM_SMALL_TILES"], defs["OD_GEMM_QUARTER_TILES_F32"], defs["OD_GEMM_BIG_MIN_M"]) == (GPU_TH.small, GPU_TH.quarter, GPU_TH.big_m)
    assert defs["OD_TN_BIG_MIN_TILES"] == TN_BIG_MIN_TILES
    emu = open(os.path.join(REPO, "tests", "emu", "build_emu.sh")).read()
    flags = {k: int(v) for k, v in re.findall(r"-D(OD_\w+)=(\d+)", emu)}
    assert (flags["OD_GEMM_SMALL_TILES"], flags["OD_GEMM_QUARTER_TILES_F32"], flags["OD_GEMM_BIG_MIN_M"]) == (EMU_TH.small, EMU_TH.quarter, EMU_TH.big_m)
    assert "inline int od_num_cus() { return %d; }" % EMU_TH.cus in open(os.path.join(CSRC, "od_api_internal.h")).read()
    for s in ("const bool half = ((M + 127) / 128) * tiles_n < OD_GEMM_SMALL_TILES;",
              "const bool quarter = f32 && ((M + 63) / 64) * tiles_n < OD_GEMM_QUARTER_TILES_F32;",
              "const bool dma = (K % (128 / (int)sizeof(T))) == 0;",
              "const bool big_rope = epi == OD_EPI_QKROPE && std::is_same<T, bf16_t>::value && rp.hd == 64 && rp.n_rope % 64 == 0 && N % 64 == 0 &&",
              "if ((epi != OD_EPI_QKROPE || big_rope) && dma && M >= OD_GEMM_BIG_MIN_M && N % 8 == 0 && ldc % 8 == 0 && N >= 256) {",
              "if (!accumulate && K % 128 == 0) {",
              "int pgrid = od_num_cus() & ~7;",
              "dim3(grid2 < pgrid ? grid2 : pgrid)",
              "if (quarter) NT_GO(EPI_, DMA_, f32 ? 1 : 2); else if (half) NT_GO(EPI_, DMA_, 2); else NT_GO(EPI_, DMA_, 4);",
              "return (DMA && WMT <= 2 && !std::is_same<T, float>::value) ? 3 : 2;",
              "if (dtype == OD_BF16 && hd == 64 && M >= OD_GEMM_BIG_MIN_M && K % 64 == 0 && N % 64 == 0 && N >= 256 && (!f16 || K % 128 == 0)) {",
              "if (K % 32) return OD_ERR_ALIGN;",
              "if (M >= OD_GEMM_BIG_MIN_M && N >= 256 && K >= 256 && (tiles2 >= OD_TN_BIG_MIN_TILES || OD_GEMM_BIG_MIN_M < 32768)) {",
              "const int target_wgs = (tiles <= 8 && M >= OD_GEMM_BIG_MIN_M) ? 512 : 2048;"):
        assert s in src, s
    # every row, and nothing but rows
    assert len(set(ROWS)) == len(ROWS)
    gpu, emu_rows = _gpu_rows(), _emu_rows()
    assert gpu <= set(ROWS) and emu_rows <= set(ROWS), (gpu | emu_rows) - set(ROWS)
    assert set(ROWS) - gpu == set(), sorted(set(ROWS) - gpu)
    assert set(ROWS) - emu_rows == set(GPU_ONLY_ROWS), sorted(set(ROWS) - emu_rows)
    for T, M, N, K in EXISTING_EMU:
        assert nt_path(T, M, N, K, th=EMU_TH).row in ROWS
    # the edges of the GPU thresholds
    gp = {c.id: c.path(GPU_TH) for c in GPU_CASES}
    assert {c.M for c in GPU_CASES if c.T == "bf16" and c.N == 264 and c.epi == "none"} >= {32767}
    assert gp[NT("bf16", 32767, 264, 128, "none", "integer").id].row == "nt/bf16/w4/dma/none"
    assert gp[NT("bf16", 32768, 256, 128, "none", "integer").id].row == "w4/none"
    assert gp[NT("bf16", 3969, 2048, 192, "none", "integer").id].wmt == 4 and gp[NT("bf16", 9343, 832, 256, "none", "integer").id].wmt == 2
    assert gp[NT("fp32", 38336, 128, 64, "none", "integer").id].wmt == 1 and gp[NT("fp32", 38337, 128, 64, "none", "integer").id].wmt == 2
    assert {p.grid for p in gp.values() if p.row == "w4/none"} == {"persistent", "one-round"}
    assert {c.path(EMU_TH).grid for c in SMALL if c.path(EMU_TH).row == "w4/none"} == {"persistent", "one-round"}
    assert any(c.N >= 1024 and c.path().kernel != "gemm_nt_kernel" for c in GPU_CASES)
    # every 128-row-kernel row with M % tile in {1, tile - 1}, its k-slab counts and an exact (integer) case, on the emulator
    for r in NT_ROWS:
        cs = [c for c in SMALL if c.path(EMU_TH).row == r]
        tile = cs[0].path(EMU_TH).tile[0]
        if r.endswith("/none"):
            assert {c.M % tile for c in cs} >= {1, tile - 1}, (r, {c.M % tile for c in cs})
            p = cs[0].path(EMU_TH)
            want = set(slab_counts(p.T, p.wmt, p.dma))
            assert want <= {c.K for c in cs if c.fam == "integer"}, (r, want)
    # TN / colsum: deterministic shadow on and off for every row
    for r in TN_ROWS:
        for on in (False, True):
            assert any(c.path(EMU_TH).row == r and c.det == on for c in TN_SMALL), (r, on)
            assert any(c.path(GPU_TH).row == r and c.det == on for c in TN_SMALL + TN_GPU), (r, on)


@pytest.mark.parametrize("case", SMALL, ids=lambda c: c.id)
def test_gemm_nt_path_small(dev, case):
    run_nt(case, dev)


@pytest.mark.parametrize("case", TN_SMALL, ids=lambda c: c.id)
def test_gemm_tn_path_small(dev, case):
    run_tn(case, dev)


@pytest.mark.parametrize("T,M,N", COLSUM_SMALL)
@pytest.mark.parametrize("on", [False, True], ids=["det-off", "det-on"])
def test_colsum_path_small(dev, T, M, N, on):
    run_colsum(T, M, N, on, dev)


@pytest.fixture(scope="module")
def gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs the GPU")
    _lib._lib = None
    _lib.lib()
    return torch.device("cuda:0")


@pytest.mark.gpu
@pytest.mark.parametrize("case", GPU_CASES, ids=lambda c: c.id)
def test_gemm_nt_path_large(gpu, case):
    run_nt(case, gpu, twice=True)


@pytest.mark.gpu
@pytest.mark.parametrize("case", TN_GPU, ids=lambda c: c.id)
def test_gemm_tn_path_large(gpu, case):
    run_tn(case, gpu, twice=True)


@pytest.mark.gpu
@pytest.mark.parametrize("T,M,N", COLSUM_GPU)
@pytest.mark.parametrize("on", [False, True], ids=["det-off", "det-on"])
def test_colsum_path_large(gpu, T, M, N, on):
    run_colsum(T, M, N, on, gpu)
