"""Every per-frame (row) kernel and the depthwise conv, against an fp64 reference computed from the same rounded operands, frame by frame,
and every cross-frame gradient sum element by element, on inputs built to reach the places where a row kernel goes wrong.

Dispatch table (osu_dreamer_amd/csrc/rowops.hip: od_rmsnorm_*, od_swiglu_rmsnorm*, od_final_norm_proj_out*, od_qk_norm_rope*;
misc.hip: od_dwconv*, od_proj_in*).  `row_path()`, `fd_path()`, `swiglu_path()`, `final_path()`, `qk_path()`, `dw_path()` and `dwb_path()` below
mirror those rules; `test_row_dispatch_table_matches_sources` re-reads the thresholds and the launcher conditions from the sources and
checks that the cases of this file still reach every row, on the GPU and on the emulator.
Thresholds: nch_for(C) = ceil(C / 512); ROWS_PER_WAVE_BWD 16 (4 waves: 64 frames of one batch row per backward block); OD_QK_BPW 8;
DW_RUN_BWD 64; OD_DW_SMALL_THREADS 131072 (emulator 10); OD_FD_SMALL_RUNS 2048 (emulator 8).  T = bf16 / fp32.

  row                                    kernel                                      selected when
  film/T/nch{1,2,3}/cl-{none,frame,bcast}   rmsnorm_film_kernel<T, NCH>               od_rmsnorm_film; cl NULL, one row per frame or per position
  film_bwd/T/nch{1,2,3}                  rmsnorm_film_bwd_kernel<T, NCH>             od_rmsnorm_film_bwd (grid ceil(L / 64) x B)
  gate/T/nch{1,2,3}                      rmsnorm_gate_res_kernel<T, NCH>             od_rmsnorm_gate_residual
  gate_bwd/T/nch{1,2,3}                  rmsnorm_gate_res_bwd_kernel<T, NCH>         od_rmsnorm_gate_residual_bwd (grid ceil(L / 64) x B)
  gate_film/T/nch{1,2,3}/cl-...          rmsnorm_gate_res_film_kernel<T, NCH>        od_rmsnorm_gate_residual_film
  film_dwconv/T/run{8,32}/ks{3,5,7,9}    rmsnorm_gate_res_film_dwconv_kernel<T,KS,RUN>  C <= 512; RUN 8 when B ceil(L / 32) < OD_FD_SMALL_RUNS; h2 NULL or not
  swiglu/T/nch{1,2,3}, swiglu_bwd/...    swiglu_rmsnorm{,_bwd}_kernel<T, NCH>        NCH = nch_for(Hp), Hf <= Hp
  final_proj/T/nch{1,2}                  final_proj_kernel<T, NCH>                   C <= 1024, E <= 8
  final_proj_bwd/T                       final_proj_bwd_kernel<T, 1>                 C <= 512, E <= 8
  qk_pos/T/lph{4,8}/nit{2,4,8}/bpw{8,<8}  qk_norm_rope_pos_kernel<T, LPH, NIT>       not f16, hd / 8 in {4, 8}, H hd / 8 % 64 = 0, ld >= 2 H hd;
                                                                                     bpw = min(B, OD_QK_BPW), lpw = OD_QK_BPW / bpw
  qk_bwd_pos/T/lph../nit../bpw..         qk_norm_rope_pos_bwd_kernel<T, LPH, NIT>    the same without the f16 / ld conditions; lpw 4x
  qk_row/{bf16,fp32,f16}                 qk_norm_rope_kernel<T[, f16_t]>             everything else (f16: bf16 in, half out)
  qk_bwd_row/T                           qk_norm_rope_bwd_kernel<T>                  everything else
  dwconv{,_varlen}/T/run{4,32}/ks{3,5,7,9}  dwconv_kernel<T, KS, RUN[, VL]>          RUN 4 when B (C / 8) ceil(L / 32) < OD_DW_SMALL_THREADS
  dwconv_bwd/T/ks{3,5,7,9}               dwconv_bwd_kernel<T, KS>                    C <= 1024 at ks <= 5, C <= 512 above; 64-frame runs
  proj_in/T, proj_in_bwd/T               proj_in_kernel<T>, proj_in_bwd_kernel<T>    E <= 8 (E = 6: the vector weight load)
  uhead_fwd{,_varlen}/wpb{1,2,3,4}       uhead_fwd_kernel<VL> (heads.hip, fp32)      windows of UW 32 frames owning UOWN 30; wpb = ceil(L / 30) B / 512
                                                                                     clamped to 1 .. UWPB 4 (2 - 4: GPU only); U <= 64, U % 8 = 0, E <= 8
  uhead_bwd                              uhead_bwd_kernel                            UWPB 4 windows per block, ceil(ceil(L / 30) / 4) x B blocks
  uhead_tail{,_varlen}, uhead_tail_bwd   uhead_tail_kernel<VL>, uhead_tail_bwd_kernel  one 64-lane block per batch row
  The u-head cases take L mod 30 in {0, 1, 29} and U 8 / 64; its forward sum fsum and every gradient are cross-frame sums.

Memory contract: every output sits inside a wider NaN-prefilled buffer (column offset 8, ld > C, rows past M; flat outputs with 64 NaN
either side), every operand inside a NaN-poisoned one.  Afterwards every element outside the output is still NaN and none inside is.
Exceptions: accumulated outputs (dres, dssg, the weight gradients) are prefilled with known finite values and must come out as prefill +
sum (the parts of dssg a kernel does not own must come out bit-identical); SwiGLU's columns Hf..Hp of each half of vg and of dhh are zero
by contract (the GEMMs that produce them write them so): hh[:, Hf:Hp] and those columns of dvg must come out exactly 0.

Input families (built in fp32, rounded to the operand type; the reference reads the rounded operands back):
  random          N(0, 1) rows.
  row_scale       frame RMS spanning 2^-20 .. 2^20, checked per frame: a frame that uses another frame's inv_rms is off by a factor.
  batch_distinct  ssg, cl and conv inputs of batch row b scaled by 10^(b mod 3): batch-index mistakes (halos crossing sequences, the q/k
                  b0 / b1 split, ssg / dssg rows).
  eps             mean squares from 1e-2 eps to 1e2 eps, every fourth frame all zero (a zero frame gives exactly shift + cl forward).
  offset          a common component of 30 with std 1: mean(g x^) in the backward is a sum that cancels.
  cancel          dh = alpha x^ / (1 + s) + 1e-3 noise: the backward's projection removes almost all of dh; measured against the scale below.
  silu_extreme    SwiGLU gates of +-30 .. +-1e4: no NaN, silu and its derivative at their limits.
  long positions  RoPE positions up to 32767 (GPU) through the table of od_rope_table.
  det             det.force(True) on every kernel that passes od_det_active(): same bounds, two runs bit-identical.
dwconv frames sit on run and block borders (lengths around multiples of the RUN and of DW_RUN_BWD) and within R of both sequence ends.
"""
import math
import os
import re
from dataclasses import dataclass

import pytest
import torch

from osu_dreamer_amd import _lib, det, ops
from kernel_backend import REPO, Fenced, Flat, bits, block_errors, det_run, dev  # noqa: F401

CSRC = os.path.join(REPO, "osu_dreamer_amd", "csrc")
NAN = float("nan")
EPS = 1e-6                                   # the channel norms' eps (oracle rms_norm_channels), passed to the kernels as fp32
EPS32 = float(torch.tensor(EPS, dtype=torch.float32))
HEPS = torch.finfo(torch.float32).eps        # the head norm's eps (q/k)
TORCH = {"bf16": torch.bfloat16, "fp32": torch.float32}


@dataclass(frozen=True)
class Th:
    fd_small: int     # OD_FD_SMALL_RUNS
    dw_small: int     # OD_DW_SMALL_THREADS


GPU_TH = Th(2048, 131072)                    # rowops.hip / misc.hip defaults: checked against the sources below
EMU_TH = Th(8, 10)                           # tests/emu/build_emu.sh
QK_BPW, RPW_BWD, DW_RUN_BWD = 8, 16, 64
UW, UOWN, UWPB = 32, 30, 4                   # heads.hip: u-head window (frames), owned frames, windows per block


def cdiv(a, b):
    return (a + b - 1) // b


def nch_for(C):
    return (C + 511) // 512


# ---------------------------------------------------------------- path functions (the table above)
def row_path(kind, T, C, cl="none"):
    r = f"{kind}/{T}/nch{nch_for(C)}"
    return f"{r}/cl-{cl}" if kind in ("film", "gate_film") else r


def fd_path(T, B, L, ks, th=GPU_TH):
    assert ks in (3, 5, 7, 9)
    return f"film_dwconv/{T}/run{8 if B * cdiv(L, 32) < th.fd_small else 32}/ks{ks}"


def swiglu_path(T, Hp, bwd):
    return f"swiglu{'_bwd' if bwd else ''}/{T}/nch{nch_for(Hp)}"


def final_path(T, C, bwd):
    assert C <= (512 if bwd else 1024)
    return f"final_proj_bwd/{T}" if bwd else f"final_proj/{T}/nch{nch_for(C)}"


def qk_path(T, B, H, hd, bwd):
    lph = hd // 8
    nit = 2 * H * lph // 64
    if T != "f16" and lph in (4, 8) and (H * lph) % 64 == 0 and nit in (2, 4, 8):      # ld >= 2 H hd holds for every case here
        return f"qk{'_bwd' if bwd else ''}_pos/{T}/lph{lph}/nit{nit}/bpw{'8' if min(B, QK_BPW) == QK_BPW else '<8'}"
    return f"qk{'_bwd' if bwd else ''}_row/{T}"


def dw_path(T, B, L, C, ks, varlen=False, th=GPU_TH):
    small = B * (C // 8) * cdiv(L, 32) < th.dw_small
    return f"dwconv{'_varlen' if varlen else ''}/{T}/run{4 if small else 32}/ks{ks}"


def dwb_path(T, C, ks):
    assert C <= 1024 and (ks <= 5 or C <= 512)
    return f"dwconv_bwd/{T}/ks{ks}"


TS = ("bf16", "fp32")
ROW_ROWS = [f"{k}/{T}/nch{n}/cl-{cl}" for k in ("film", "gate_film") for T in TS for n in (1, 2, 3) for cl in ("none", "frame", "bcast")]
ROW_ROWS += [f"{k}/{T}/nch{n}" for k in ("film_bwd", "gate", "gate_bwd") for T in TS for n in (1, 2, 3)]
FD_ROWS = [f"film_dwconv/{T}/run{r}/ks{k}" for T in TS for r in (8, 32) for k in (3, 5, 7, 9)]
SW_ROWS = [f"swiglu{b}/{T}/nch{n}" for b in ("", "_bwd") for T in TS for n in (1, 2, 3)]
FIN_ROWS = [f"final_proj/{T}/nch{n}" for T in TS for n in (1, 2)] + [f"final_proj_bwd/{T}" for T in TS]
QK_ROWS = [f"qk{b}_pos/{T}/lph{l}/nit{n}/bpw{w}" for b in ("", "_bwd") for T in TS for l in (4, 8) for n in (2, 4, 8) for w in ("8", "<8")]
QK_ROWS += ["qk_row/bf16", "qk_row/fp32", "qk_row/f16", "qk_bwd_row/bf16", "qk_bwd_row/fp32"]
DW_ROWS = [f"dwconv{v}/{T}/run{r}/ks{k}" for v in ("", "_varlen") for T in TS for r in (4, 32) for k in (3, 5, 7, 9)]
DW_ROWS += [f"dwconv_bwd/{T}/ks{k}" for T in TS for k in (3, 5, 7, 9)]
PI_ROWS = [f"proj_in{b}/{T}" for b in ("", "_bwd") for T in TS]
UH_ROWS = [f"uhead_{k}/wpb{w}" for k in ("fwd", "fwd_varlen") for w in (1, 2, 3, 4)] + ["uhead_bwd", "uhead_tail", "uhead_tail_varlen", "uhead_tail_bwd"]
ROWS = ROW_ROWS + FD_ROWS + SW_ROWS + FIN_ROWS + QK_ROWS + DW_ROWS + PI_ROWS + UH_ROWS
# rows the emulator's cases cannot reach: the u-head forward with 2 - 4 windows per block (it needs ceil(L / 30) B >= 1024 windows, a
# size the emulator runs too slowly; the backward always walks 4 windows per block and runs there).  Its thresholds put both RUN choices
# of the conv kernels within reach of small shapes.
GPU_ONLY_ROWS = [f"uhead_{k}/wpb{w}" for k in ("fwd", "fwd_varlen") for w in (2, 3, 4)]

# ---------------------------------------------------------------- bounds
# Per frame: relative L2 of (kernel - fp64 reference) over the frame's row, against the reference row or a stated scale row.
#   bf16 outputs: one rounding to 8 significant bits, <= 2^-8 of each element, so <= 2^-8 of the frame in relative L2 — a hard bound
#     (typical ~2^-9.5); the fp32 arithmetic before it adds a few 2^-24.  fp32 outputs: the frame's sum of squares is <= 30 sequential fp32
#     additions per lane + tree (24 chunks of 8 at C = 1536, 6 shuffle levels): <= 30 2^-24 of it, half that in rsqrt; the products and the
#     output add a few more: 2^-17 (128 2^-24) leaves a margin of four.
#   Accumulated outputs (dres += ...) and families that cancel are measured against a scale: |old| + inv (|g| + |x^| mean|g x^|) for the
#     norm backwards (the magnitudes the fp32 terms carry before they cancel), sum_j |w_j| |x| + |b| for the conv.
OUT = {"bf16": 2.0 ** -8 + 2.0 ** -16, "fp32": 2.0 ** -17}
# inv_rms per element: the sum of squares above (<= 30 2^-24 relative), halved by the rsqrt, plus its own ulp and the division by C.
INV_B = 2.0 ** -19


# Cross-frame sums per element (dssg, dwq / dwk, dW / db, the conv taps, the u-head gradients), measured against |old| + sum |terms| — in
# bf16 mode too: the inputs are rounded, the sums are not.  The terms are fp32 products of rounded operands (a few roundings each, 2^-24).
# Inside a block the sum is a fixed chain of fp32 additions (the rows a lane adds in registers, then the block's reduction steps): each
# rounds by <= 2^-24 of its partial sum <= sum |terms|, so `inner` additions cost <= inner 2^-24, a hard bound (+ 4 for the per-term
# roundings).  The block partials then meet in one address by atomics, in any order: each addition rounds by an error uniform in +-2^-24
# of its partial (standard deviation 2^-24 / sqrt 3), so over `blocks` partials the random walk stays within 4 sqrt(blocks / 3) 2^-24.
# At the bench shape: 128 blocks per batch row (dssg) -> 3e-6; 4096 blocks (dW of the final projection) -> 1e-5.
# The fixed-point sums (od_lds_fix_add and the deterministic shadow, step 2^-40, rounded to nearest) add <= 2^-41 per contribution: an
# absolute floor of n 2^-41.
def sum_bound(inner, blocks):
    return (inner + 4) * 2.0 ** -24 + 4 * math.sqrt(blocks / 3) * 2.0 ** -24


def fix_floor(n):
    return n * 2.0 ** -41


# ---------------------------------------------------------------- checks
def check_frames(case, what, out, ref, bound, scale=None):
    """Relative L2 per frame (row of the frame-major layout), with no floor: every frame counts as much as any other."""
    blk, glob = block_errors(out.reshape(ref.shape[0], -1), ref.reshape(ref.shape[0], -1), rows=1, floor=0.0, floor_max=0.0,
                             scale=None if scale is None else scale.reshape(ref.shape[0], -1))
    blk = torch.nan_to_num(blk.flatten(), nan=float("inf"))
    worst = int(blk.argmax())
    assert float(blk[worst]) <= bound, f"{case} {what}: frame {worst} error {float(blk[worst]):.3e} > {bound:.3e} (global {glob:.3e})"
    return float(blk[worst])


def check_elems(case, what, out, ref, absterms, bound, floor=0.0):
    err = (out.double() - ref).abs()
    lim = bound * absterms + floor
    bad = ~(err <= lim)
    if bool(bad.any()):
        i = tuple(int(j) for j in bad.nonzero()[0])
        raise AssertionError(f"{case} {what}: {int(bad.sum())} elements off, first {i}: {float(out.double()[i]):.9e} against "
                             f"{float(ref[i]):.9e}, error {float(err[i]):.3e} / sum|terms| {float(absterms[i]):.3e} > {bound:.3e}")


def check_inv(case, inv, ref):
    rel = ((inv.double() - ref).abs() / ref)
    assert bool((rel <= INV_B).all()), f"{case} inv_rms: worst {float(torch.nan_to_num(rel, nan=float('inf')).max()):.3e} > {INV_B:.3e}"


# ---------------------------------------------------------------- operands
def _gen(device, seed):
    return torch.Generator(device=device).manual_seed(seed)


def frame_rows(fam, B, L, C, g, device):
    """fp32 (B L, C) rows of the family."""
    M = B * L
    rn = torch.randn(M, C, generator=g, device=device)
    if fam == "row_scale":
        return rn * 2.0 ** torch.randint(-20, 21, (M, 1), generator=g, device=device).float()
    if fam == "batch_distinct":
        return rn * batch_scale(B, L, device)[:, None]
    if fam == "eps":
        ms = EPS * 10.0 ** (4 * torch.rand(M, 1, generator=g, device=device) - 2)
        x = rn / rn.pow(2).mean(1, keepdim=True).sqrt() * ms.sqrt()
        x[::4] = 0
        return x
    if fam == "offset":
        return 30 + rn
    return rn


def batch_scale(B, L, device):
    return (10.0 ** (torch.arange(B, device=device) % 3).float()).repeat_interleave(L)


def ssg_of(fam, B, C, g, device):
    s = 0.5 * torch.randn(B, 3 * C, generator=g, device=device)
    if fam == "batch_distinct":
        s = s * (10.0 ** (torch.arange(B, device=device) % 3).float())[:, None]
    return s


def rd(t, T):
    """Round fp32 to the operand type and read it back as fp64 (the reference's operand)."""
    return t.to(TORCH[T]).double()


# ---------------------------------------------------------------- row cases
@dataclass(frozen=True)
class RC:
    kind: str                 # film, film_bwd, gate, gate_bwd, gate_film, film_dwconv
    T: str
    B: int
    L: int
    C: int
    fam: str = "random"
    cl: str = "none"          # none / frame / bcast (film, gate_film)
    ks: int = 5               # film_dwconv
    h2: bool = True           # film_dwconv: h2 written (training) or NULL
    det: bool = False
    seed: int = 0

    @property
    def id(self):
        ex = (f"-cl{self.cl}" if self.cl != "none" else "") + (f"-ks{self.ks}{'' if self.h2 else '-noh2'}" if self.kind == "film_dwconv" else "")
        return f"{self.kind}-{self.T}-{self.fam}{ex}{'-det' if self.det else ''}-{self.B}x{self.L}x{self.C}"

    def path(self, th=GPU_TH):
        if self.kind == "film_dwconv":
            return fd_path(self.T, self.B, self.L, self.ks, th)
        return row_path(self.kind, self.T, self.C, self.cl)


def norm_ref(xd):
    """inv_rms in fp64 of the rounded rows, eps inside the channel mean (oracle rms_norm_channels)."""
    return torch.rsqrt(xd.pow(2).mean(1) + EPS32)


def run_row(c: RC, device, twice=False):
    T, B, L, C = c.T, c.B, c.L, c.C
    tt = TORCH[T]
    M = B * L
    g = _gen(device, 11 + c.seed)
    bi = torch.arange(M, device=device) // L
    case = f"{c.id} [{c.path()}]"
    x32 = frame_rows(c.fam, B, L, C, g, device)
    xin = Fenced(M, C, tt, device, x32)
    xd = xin.v.double()
    ssg = Flat((B, 3 * C), device, ssg_of(c.fam, B, C, g, device))
    sd = ssg.v.double()
    s, sh, gate = sd[bi, :C], sd[bi, C:2 * C], sd[bi, 2 * C:]

    if c.kind in ("film", "gate", "gate_film", "film_dwconv"):
        cl = cld = None
        if c.cl != "none":
            nr = L if c.cl == "bcast" else M
            c32 = torch.randn(nr, C, generator=g, device=device)
            if c.fam == "batch_distinct" and c.cl == "frame":
                c32 = c32 * batch_scale(B, L, device)[:, None]
            cl = Fenced(nr, C, tt, device, c32)
            cld = cl.v.double()[torch.arange(M, device=device) % L] if c.cl == "bcast" else cl.v.double()
        if c.kind == "film":
            h = Fenced(M, C, tt, device)
            inv = Flat((M,), device)
            ops.rmsnorm_film(xin.v, ssg.v, None if cl is None else cl.v, c.cl == "bcast", h.v, inv.v, B, L, eps=EPS)
            h.check(case, "h")
            inv.check(case, "inv_rms")
            invd = norm_ref(xd)
            check_inv(case, inv.v, invd)
            ref = xd * invd[:, None] * (1 + s) + sh + (0 if cld is None else cld)
            check_frames(case, "h", h.v, ref, OUT[T])
            z = xd.abs().sum(1) == 0
            if bool(z.any()):           # zero frames: exactly shift (+ cl), the fp32 sum rounded once to the output type
                want = (ssg.v[bi, C:2 * C] + (0 if cl is None else cld.float()))[z].to(tt)
                assert torch.equal(h.v[z], want), f"{case}: a zero frame is not exactly shift + cl"
            return
        # gate / gate_film / film_dwconv: x is the residual stream, h the branch output being normalised
        h32 = frame_rows(c.fam, B, L, C, g, device)
        hin = Fenced(M, C, tt, device, h32)
        hd = hin.v.double()
        inv_h = norm_ref(hd)
        xo = Fenced(M, C, tt, device)
        inv_a = Flat((M,), device)
        ref_xo = xd + hd * inv_h[:, None] * gate
        if c.kind == "gate":
            ops.rmsnorm_gate_residual(xin.v, hin.v, ssg.v, xo.v, inv_a.v, B, L, eps=EPS)
        else:
            ssg_b = Flat((B, 3 * C), device, ssg_of(c.fam, B, C, g, device))
            sbd = ssg_b.v.double()
            inv_b, h2 = Flat((M,), device), Fenced(M, C, tt, device)
            if c.kind == "gate_film":
                ops.rmsnorm_gate_residual_film(xin.v, hin.v, ssg.v, xo.v, inv_a.v, ssg_b.v, None if cl is None else cl.v, c.cl == "bcast",
                                               h2.v, inv_b.v, B, L, eps=EPS)
            else:
                cw = Flat((C, 1, c.ks), device, 0.4 * torch.randn(C, 1, c.ks, generator=g, device=device))
                cb = Flat((C,), device, torch.randn(C, generator=g, device=device))
                y = Fenced(M, C, tt, device)
                ops.rmsnorm_gate_residual_film_dwconv(xin.v, hin.v, ssg.v, xo.v, inv_a.v, ssg_b.v, h2.v if c.h2 else None, inv_b.v, cw.v,
                                                      cb.v, y.v, B, L, c.ks, eps=EPS)
            # the second norm reads xo as rounded to T (the kernel's own xo, itself checked below)
            xod = xo.v.double()
            inv2 = norm_ref(xod)
            ref_h2 = xod * inv2[:, None] * (1 + sbd[bi, :C]) + sbd[bi, C:2 * C] + (0 if cld is None else cld)
            inv_b.check(case, "inv_b")
            check_inv(case + " (second norm)", inv_b.v, inv2)
            if c.kind == "gate_film" or c.h2:
                h2.check(case, "h2")
                check_frames(case, "h2", h2.v, ref_h2, OUT[T])
            else:
                assert bool(torch.isnan(h2.buf.float()).all()), f"{case}: h2 is NULL but something was written"
            if c.kind == "film_dwconv":
                y.check(case, "y")
                # y = conv(h2 as rounded to T): with h2 written, exactly the kernel's h2; with NULL, the reference's h2 rounded to T (an
                # element that sits on a rounding midpoint may differ by one ulp: one more 2^-8 of one tap, covered by measuring against
                # sum |w| |h2| + |b|)
                h2r = h2.v.double() if c.h2 else ref_h2.to(tt).double()
                ref_y, sc_y = conv_ref(h2r, cw.v.double(), cb.v.double(), B, L, c.ks)
                check_frames(case, "y", y.v, ref_y, OUT[T] + (0 if c.h2 else 2.0 ** -8), sc_y)
        xo.check(case, "xo")
        inv_a.check(case, "inv_rms")
        check_inv(case, inv_a.v, inv_h)
        check_frames(case, "xo", xo.v, ref_xo, OUT[T], xd.abs() + (hd * inv_h[:, None] * gate).abs())
        return

    # backwards: inv_rms as the forward stores it (fp32 of the exact value); accumulated outputs prefilled
    src = xd
    invf = norm_ref(src).float()
    inv = Flat((M,), device, invf)
    invd = inv.v.double()
    xh = src * invd[:, None]
    mult = (1 + s) if c.kind == "film_bwd" else gate
    dh32 = torch.randn(M, C, generator=g, device=device)
    if c.fam == "cancel":
        alpha = torch.randn(M, 1, generator=g, device=device, dtype=torch.float64)
        dh32 = (alpha * xh / mult).float() + 1e-3 * dh32
    dhin = Fenced(M, C, tt, device, dh32)
    dhd = dhin.v.double()
    gg = dhd * mult
    dot = (gg * xh).mean(1, keepdim=True)
    delta = invd[:, None] * (gg - xh * dot)
    scale = invd[:, None] * (gg.abs() + xh.abs() * (gg * xh).abs().mean(1, keepdim=True))
    old = (0.5 * torch.randn(M, C, generator=g, device=device, dtype=torch.float64) * scale.pow(2).mean(1, keepdim=True).sqrt()).to(tt)
    dssg0 = torch.randn(B, 3 * C, generator=g, device=device)

    def launch():
        dssg = Flat((B, 3 * C), device, dssg0)
        out = Fenced(M, C, tt, device, old if c.kind == "film_bwd" else None)
        if c.kind == "film_bwd":
            det_run(device, c.det, [dssg.v], lambda: ops.rmsnorm_film_bwd(xin.v, inv.v, ssg.v, dhin.v, out.v, dssg.v, B, L))
        else:
            det_run(device, c.det, [dssg.v], lambda: ops.rmsnorm_gate_residual_bwd(xin.v, inv.v, ssg.v, dhin.v, out.v, dssg.v, B, L))
        return dssg, out

    dssg, out = launch()
    out.check(case, "dres" if c.kind == "film_bwd" else "dh")
    dssg.check(case, "dssg")
    if c.kind == "film_bwd":
        check_frames(case, "dres", out.v, old.double() + delta, OUT[T], old.double().abs() + scale)
        own = slice(0, 2 * C)
        terms = torch.cat([dhd * xh, dhd], 1)
    else:
        check_frames(case, "dh", out.v, delta, OUT[T], scale)
        own = slice(2 * C, 3 * C)
        terms = dhd * xh
    d0 = dssg0.double()
    ref = d0[:, own] + torch.zeros(B, terms.shape[1], dtype=torch.float64, device=device).index_add_(0, bi, terms)
    absterms = d0[:, own].abs() + torch.zeros_like(ref).index_add_(0, bi, terms.abs())
    # a lane adds its wave's 16 rows, the block's 4 waves meet in LDS, then one atomic per block of 64 frames
    check_elems(case, "dssg", dssg.v[:, own], ref, absterms, sum_bound(RPW_BWD + 4, cdiv(L, 4 * RPW_BWD)),
                fix_floor(cdiv(L, 4 * RPW_BWD)) if c.det else 0.0)
    rest = torch.ones(3 * C, dtype=torch.bool, device=device)
    rest[own] = False
    assert torch.equal(dssg.v[:, rest], dssg0[:, rest]), f"{case}: dssg columns the kernel does not own were changed"
    if twice or c.det:
        dssg2, out2 = launch()
        if c.det:
            assert torch.equal(bits(dssg2.buf), bits(dssg.buf)) and torch.equal(bits(out2.buf), bits(out.buf)), f"{case}: two runs differ"


def conv_ref(xd, wd, bd, B, L, ks):
    """Depthwise conv along frames with zero padding at both sequence ends: y, and the scale sum_j |w_j| |x| + |b|."""
    R = ks // 2
    C = xd.shape[1]
    xp = torch.nn.functional.pad(xd.reshape(B, L, C), (0, 0, R, R))
    w = wd.reshape(C, ks)
    y = bd.expand(B, L, C).clone()
    sc = bd.abs().expand(B, L, C).clone()
    for j in range(ks):
        y += w[:, j] * xp[:, j:j + L]
        sc += w[:, j].abs() * xp[:, j:j + L].abs()
    return y.reshape(B * L, C), sc.reshape(B * L, C)


# ---------------------------------------------------------------- SwiGLU
@dataclass(frozen=True)
class SW:
    T: str
    M: int
    Hf: int
    Hp: int
    fam: str = "random"
    bwd: bool = False
    seed: int = 0

    @property
    def id(self):
        return f"swiglu{'_bwd' if self.bwd else ''}-{self.T}-{self.fam}-{self.M}x{self.Hf}of{self.Hp}"

    def path(self, th=GPU_TH):
        return swiglu_path(self.T, self.Hp, self.bwd)


def run_swiglu(c: SW, device, twice=False):
    T, M, Hf, Hp = c.T, c.M, c.Hf, c.Hp
    tt = TORCH[T]
    g = _gen(device, 21 + c.seed)
    case = f"{c.id} [{c.path()}]"
    v32 = frame_rows("row_scale" if c.fam == "row_scale" else "random", 1, M, Hf, g, device)
    g32 = torch.randn(M, Hf, generator=g, device=device)
    if c.fam == "silu_extreme":
        g32 = torch.sign(g32) * 30.0 * (1e4 / 30.0) ** torch.rand(M, Hf, generator=g, device=device)
    if c.fam == "eps":
        v32 = frame_rows("eps", 1, M, Hf, g, device)
        g32 = 3 + g32.abs()                      # silu(g) ~ g: the product's mean square stays near eps
    vg = Fenced(M, 2 * Hp, tt, device, torch.zeros(M, 2 * Hp, device=device))
    vg.v[:, :Hf] = v32.to(tt)
    vg.v[:, Hp:Hp + Hf] = g32.to(tt)
    vd, gd = vg.v[:, :Hf].double(), vg.v[:, Hp:Hp + Hf].double()
    sig = torch.sigmoid(gd)
    a = vd * gd * sig
    invd = torch.rsqrt(a.pow(2).mean(1) + EPS32)
    if not c.bwd:
        hh, inv = Fenced(M, Hp, tt, device), Flat((M,), device)
        ops.swiglu_rmsnorm(vg.v, hh.v, inv.v, Hf, Hp, eps=EPS)
        hh.check(case, "hh")
        inv.check(case, "inv_rms")
        check_inv(case, inv.v, invd)
        assert bool((hh.v[:, Hf:] == 0).all()), f"{case}: hh[:, Hf:Hp] is not exactly 0"
        check_frames(case, "hh", hh.v[:, :Hf], a * invd[:, None], OUT[T] + 2.0 ** -19)      # + the hardware exp in silu (~2^-19 at |g| <= 30)
        return
    inv = Flat((M,), device, invd.float())
    invd = inv.v.double()
    d32 = torch.randn(M, Hf, generator=g, device=device)
    if c.fam == "cancel":       # dhh = alpha hh + 1e-3 noise: the projection removes almost all of it
        d32 = (torch.randn(M, 1, generator=g, device=device, dtype=torch.float64) * a * invd[:, None]).float() + 1e-3 * d32
    dhh = Fenced(M, Hp, tt, device, torch.zeros(M, Hp, device=device))
    dhh.v[:, :Hf] = d32.to(tt)
    dd = dhh.v[:, :Hf].double()
    shv = a * invd[:, None]
    dot = (dd * shv).sum(1, keepdim=True) / Hf
    ds = invd[:, None] * (dd - shv * dot)
    ref_v = ds * gd * sig
    ref_g = ds * vd * (sig * (1 + gd * (1 - sig)))
    sc = invd[:, None] * (dd.abs() + shv.abs() * (dd * shv).abs().mean(1, keepdim=True))     # |ds| before its projection cancels

    def launch():
        dvg = Fenced(M, 2 * Hp, tt, device)
        ops.swiglu_rmsnorm_bwd(vg.v, inv.v, dhh.v, dvg.v, Hf, Hp)
        return dvg
    dvg = launch()
    dvg.check(case, "dvg")
    assert bool((dvg.v[:, Hf:Hp] == 0).all() & (dvg.v[:, Hp + Hf:] == 0).all()), f"{case}: dvg columns Hf..Hp are not exactly 0"
    b = OUT[T] + 2.0 ** -19
    check_frames(case, "dv", dvg.v[:, :Hf], ref_v, b, sc * (gd * sig).abs())
    check_frames(case, "dg", dvg.v[:, Hp:Hp + Hf], ref_g, b, sc * (vd * (sig * (1 + gd * (1 - sig)))).abs())
    if twice:
        assert torch.equal(bits(launch().buf), bits(dvg.buf)), f"{case}: two runs differ"


# ---------------------------------------------------------------- final norm + projection
@dataclass(frozen=True)
class FP:
    T: str
    B: int
    L: int
    C: int
    E: int = 6
    fam: str = "random"
    bwd: bool = False
    det: bool = False

    @property
    def id(self):
        return f"final_proj{'_bwd' if self.bwd else ''}-{self.T}-{self.fam}-E{self.E}{'-det' if self.det else ''}-{self.B}x{self.L}x{self.C}"

    def path(self, th=GPU_TH):
        return final_path(self.T, self.C, self.bwd)


def run_final(c: FP, device, twice=False):
    T, B, L, C, E = c.T, c.B, c.L, c.C, c.E
    tt = TORCH[T]
    M = B * L
    g = _gen(device, 31)
    case = f"{c.id} [{c.path()}]"
    W = Flat((E, C, 1), device, 0.3 * torch.randn(E, C, 1, generator=g, device=device))
    bias = Flat((E,), device, torch.randn(E, generator=g, device=device))
    coef = torch.randn(M, E, generator=g, device=device)
    if c.fam == "cancel":       # x in the span of W's rows and dv = alpha coef: dv W is alpha x (+ 1e-3 noise), which the projection removes
        xin = Fenced(M, C, tt, device, coef @ W.v.reshape(E, C) + 1e-3 * torch.randn(M, C, generator=g, device=device))
    else:
        xin = Fenced(M, C, tt, device, frame_rows(c.fam, B, L, C, g, device))
    xd = xin.v.double()
    Wd, bd = W.v.double().reshape(E, C), bias.v.double()
    invd = norm_ref(xd)
    if not c.bwd:
        v, inv = Flat((B, E, L), device), Flat((M,), device)
        ops.final_norm_proj_out(xin.v, W.v, bias.v, v.v, inv.v, B, L, eps=EPS)
        v.check(case, "v")
        inv.check(case, "inv_rms")
        check_inv(case, inv.v, invd)
        ref = (xd * invd[:, None]) @ Wd.t() + bd
        sc = (xd.abs() * invd[:, None]) @ Wd.abs().t() + bd.abs()
        # fp32 output of fp32 sums in both modes: per frame (the E values of frame (b, l)) against sum |w| |x^| + |b|
        check_frames(case, "v", v.v.permute(0, 2, 1).reshape(M, E), ref, OUT["fp32"], sc)
        return
    inv = Flat((M,), device, invd.float())
    invd = inv.v.double()
    xh = xd * invd[:, None]
    dv32 = torch.randn(B, E, L, generator=g, device=device)
    if c.fam == "cancel":
        dv32 = (torch.randn(M, 1, generator=g, device=device) * coef).reshape(B, L, E).permute(0, 2, 1)
    dv = Flat((B, E, L), device, dv32)
    dvf = dv.v.double().permute(0, 2, 1).reshape(M, E)
    dn = dvf @ Wd
    dot = (dn * xh).mean(1, keepdim=True)
    ref_dx = invd[:, None] * (dn - xh * dot)
    sc = invd[:, None] * (dvf.abs() @ Wd.abs() + xh.abs() * (dn * xh).abs().mean(1, keepdim=True))
    dW0, db0 = torch.randn(E, C, 1, generator=g, device=device), torch.randn(E, generator=g, device=device)

    def launch():
        dx, dW, db = Fenced(M, C, tt, device), Flat((E, C, 1), device, dW0), Flat((E,), device, db0)
        det_run(device, c.det, [dW.v, db.v], lambda: ops.final_norm_proj_out_bwd(xin.v, inv.v, W.v, dv.v, dx.v, dW.v, db.v, B, L))
        return dx, dW, db
    dx, dW, db = launch()
    dx.check(case, "dx")
    dW.check(case, "dW")
    db.check(case, "db")
    check_frames(case, "dx", dx.v, ref_dx, OUT[T], sc)
    nb = B * cdiv(L, 4 * RPW_BWD)                    # blocks meeting in each dW / db address
    fl = fix_floor(nb) if c.det else 0.0
    check_elems(case, "dW", dW.v.reshape(E, C), dW0.double().reshape(E, C) + dvf.t() @ xh,
                dW0.double().abs().reshape(E, C) + dvf.abs().t() @ xh.abs(), sum_bound(RPW_BWD + 4, nb), fl)
    check_elems(case, "db", db.v, db0.double() + dvf.sum(0), db0.double().abs() + dvf.abs().sum(0), sum_bound(RPW_BWD + 4, nb), fl)
    if twice or c.det:
        dx2, dW2, db2 = launch()
        if c.det:
            assert all(torch.equal(bits(p.buf), bits(q.buf)) for p, q in ((dx, dx2), (dW, dW2), (db, db2))), f"{case}: two runs differ"


# ---------------------------------------------------------------- q/k norm + RoPE
@dataclass(frozen=True)
class QK:
    T: str                    # bf16, fp32, f16 (bf16 in, half out: forward only)
    B: int
    L: int
    H: int
    hd: int
    fam: str = "random"
    qs: float = 1.0
    bwd: bool = False
    det: bool = False

    @property
    def id(self):
        return f"qk{'_bwd' if self.bwd else ''}-{self.T}-{self.fam}-qs{self.qs:g}{'-det' if self.det else ''}-{self.B}x{self.L}-H{self.H}x{self.hd}"

    def path(self, th=GPU_TH):
        return qk_path(self.T, self.B, self.H, self.hd, self.bwd)


def run_qk(c: QK, device, twice=False):
    B, L, H, hd = c.B, c.L, c.H, c.hd
    M, dh, half = B * L, H * hd, hd // 2
    T_in = "bf16" if c.T == "f16" else c.T
    tt = TORCH[T_in]
    g = _gen(device, 41)
    case = f"{c.id} [{c.path()}]"
    # the v columns of qkv stay NaN: the kernels must not read them
    qkv = Fenced(M, 3 * dh, tt, device)
    qkv.v[:, :2 * dh] = frame_rows(c.fam, B, L, 2 * dh, g, device).to(tt)
    q_in = qkv.v[:, :2 * dh]
    xd = q_in.double().reshape(M, 2, H, hd)
    wq = Flat((hd,), device, 1 + 0.2 * torch.randn(hd, generator=g, device=device))
    wk = Flat((hd,), device, 1 + 0.2 * torch.randn(hd, generator=g, device=device))
    tab = Flat((L, half, 2), device)
    ops.rope_table(tab.v, L, hd)
    tab.check(case, "rope table")
    pos = torch.arange(M, device=device) % L
    td = tab.v.double()
    cs, sn = td[pos, :, 0][:, None, None, :], td[pos, :, 1][:, None, None, :]
    w = torch.stack([wq.v.double(), wk.v.double()])[None, :, None, :]                 # (1, 2, 1, hd)
    sgain = torch.tensor([c.qs, 1.0], dtype=torch.float64, device=device)[None, :, None, None]
    inv = torch.rsqrt(xd.pow(2).mean(-1, keepdim=True) + HEPS)
    xh = xd * inv
    if not c.bwd:
        y = xh * w
        a, b = y[..., :half], y[..., half:]
        ref = (torch.cat([a * cs - b * sn, a * sn + b * cs], -1) * sgain).reshape(M, 2 * dh)
        ot = torch.float16 if c.T == "f16" else tt
        out = Fenced(M, 2 * dh, ot, device)
        if c.T == "f16":
            _lib.lib().od_qk_norm_rope(_lib.OD_F16, q_in.data_ptr(), q_in.stride(0), wq.v.data_ptr(), wk.v.data_ptr(), tab.v.data_ptr(),
                                       out.v.data_ptr(), out.v.stride(0), B, L, H, hd, HEPS, c.qs, ops._stream(q_in))
        else:
            ops.qk_norm_rope(q_in, wq.v, wk.v, tab.v, out.v, B, L, H, hd, HEPS, q_scale=c.qs)
        out.check(case, "qk")
        check_frames(case, "q/k", out.v, ref, OUT["bf16"] if c.T == "bf16" else 2.0 ** -11 + 2.0 ** -17 if c.T == "f16" else OUT["fp32"])
        return
    d32 = torch.randn(M, 2 * dh, generator=g, device=device)
    if c.fam == "cancel":       # dqk = the rotation of alpha x^ / w (+ 1e-3 noise): d x^ = alpha x^, which the projection removes
        uc = torch.randn(M, 1, 1, 1, generator=g, device=device, dtype=torch.float64) * xh / w
        u1, u2 = uc[..., :half], uc[..., half:]
        d32 = (torch.cat([u1 * cs - u2 * sn, u1 * sn + u2 * cs], -1) / sgain).reshape(M, 2 * dh).float() + 1e-3 * d32
    dqk = Fenced(M, 2 * dh, tt, device, d32)
    dd = dqk.v.double().reshape(M, 2, H, hd) * sgain
    d1, d2 = dd[..., :half], dd[..., half:]
    u = torch.cat([d1 * cs + d2 * sn, -d1 * sn + d2 * cs], -1)                      # the gradient of y = x^ w (un-rotated)
    dxh = u * w
    dot = (dxh * xh).mean(-1, keepdim=True)
    ref_dx = (inv * (dxh - xh * dot)).reshape(M, 2 * dh)
    sc = (inv * (dxh.abs() + xh.abs() * (dxh * xh).abs().mean(-1, keepdim=True))).reshape(M, 2 * dh)
    gw = (u * xh).sum((0, 2))                                                          # (2, hd)
    gwa = (u * xh).abs().sum((0, 2))
    dw0 = torch.randn(2, hd, generator=g, device=device)

    def launch():
        dqkv = Fenced(M, 3 * dh, tt, device)
        dwq, dwk = Flat((hd,), device, dw0[0]), Flat((hd,), device, dw0[1])
        det_run(device, c.det, [dwq.v, dwk.v], lambda: ops.qk_norm_rope_bwd(q_in, wq.v, wk.v, tab.v, dqk.v, dqkv.v[:, :2 * dh], dwq.v, dwk.v,
                                                                             B, L, H, hd, HEPS, q_scale=c.qs))
        return dqkv, dwq, dwk
    dqkv, dwq, dwk = launch()
    assert bool(torch.isnan(dqkv.v[:, 2 * dh:].float()).all()), f"{case}: the v columns of dqkv were written"
    dqkv.rows, dqkv.cols = M, 2 * dh
    dqkv.check(case, "dqkv[:, :2 H hd]")
    dwq.check(case, "dwq")
    dwk.check(case, "dwk")
    check_frames(case, "dq/dk", dqkv.v[:, :2 * dh], ref_dx, OUT[c.T], sc)
    # the chain: a lane adds its frames x heads in registers (position-major: bpw x 4 lpw frames, NIT / 2 heads; row kernel: 16 frames x
    # its pieces), the lanes of a feature meet by shuffles (<= 4 levels), the block in fixed point, then one atomic per block
    lph, nit = hd // 8, 2 * H * (hd // 8) // 64
    if c.path().startswith("qk_bwd_pos"):
        bpw = min(B, QK_BPW)
        lpw = max(1, QK_BPW // bpw) * 4
        inner, nb = bpw * lpw * (nit // 2) + 4, cdiv(cdiv(L, lpw) * cdiv(B, bpw), 4)
    else:
        inner, nb = RPW_BWD * cdiv(2 * H * lph, 64) + 4, cdiv(M, 4 * RPW_BWD)
    for i, (name, t) in enumerate((("dwq", dwq), ("dwk", dwk))):
        check_elems(case, name, t.v, dw0[i].double() + gw[i], dw0[i].double().abs() + gwa[i], sum_bound(inner, nb), fix_floor(256 * nb))
    if twice or c.det:
        r2 = launch()
        if c.det:
            assert all(torch.equal(bits(p.buf), bits(q.buf)) for p, q in zip((dqkv, dwq, dwk), r2)), f"{case}: two runs differ"


# ---------------------------------------------------------------- depthwise conv and proj_in
@dataclass(frozen=True)
class DW:
    kind: str                 # dwconv, dwconv_varlen, dwconv_bwd
    T: str
    B: int
    L: int
    C: int
    ks: int
    fam: str = "random"
    det: bool = False

    @property
    def id(self):
        return f"{self.kind}-{self.T}-{self.fam}-ks{self.ks}{'-det' if self.det else ''}-{self.B}x{self.L}x{self.C}"

    def path(self, th=GPU_TH):
        if self.kind == "dwconv_bwd":
            return dwb_path(self.T, self.C, self.ks)
        return dw_path(self.T, self.B, self.L, self.C, self.ks, self.kind == "dwconv_varlen", th)


def run_dw(c: DW, device, twice=False):
    T, B, L, C, ks = c.T, c.B, c.L, c.C, c.ks
    tt = TORCH[T]
    M, R = B * L, ks // 2
    g = _gen(device, 51)
    case = f"{c.id} [{c.path()}]"
    x32 = torch.randn(M, C, generator=g, device=device)
    if c.fam == "batch_distinct":
        x32 = x32 * batch_scale(B, L, device)[:, None]
    xin = Fenced(M, C, tt, device, x32)
    xd = xin.v.double()
    w = Flat((C, 1, ks), device, 0.4 * torch.randn(C, 1, ks, generator=g, device=device))
    bias = Flat((C,), device, torch.randn(C, generator=g, device=device))
    wd, bd = w.v.double().reshape(C, ks), bias.v.double()
    if c.kind != "dwconv_bwd":
        y = Fenced(M, C, tt, device)
        if c.kind == "dwconv":
            ops.dwconv(xin.v, w.v, bias.v, y.v, B, L, ks)
            ref, sc = conv_ref(xd, wd, bd, B, L, ks)
        else:
            lens = torch.tensor([max(0, L - 7 * b) if b % 2 else L - b for b in range(B)], dtype=torch.int32, device=device)
            ops.dwconv_varlen(xin.v, w.v, bias.v, y.v, lens, B, L, ks)
            valid = (torch.arange(M, device=device) % L < lens.long().repeat_interleave(L))[:, None]
            ref, sc = conv_ref(xd * valid, wd, bd, B, L, ks)
            ref, sc = ref * valid, sc * valid
            assert bool((y.v[~valid[:, 0]] == 0).all()), f"{case}: frames past a sequence's end are not exactly 0"
        y.check(case, "y")
        check_frames(case, "y", y.v, ref, OUT[T], sc)
        return
    dy = Fenced(M, C, tt, device, torch.randn(M, C, generator=g, device=device))
    dyd = dy.v.double()
    # dx = the conv of dy with the taps reversed, no bias
    ref_dx, sc_dx = conv_ref(dyd, wd.flip(1), torch.zeros(C, dtype=torch.float64, device=device), B, L, ks)
    xp = torch.nn.functional.pad(xd.reshape(B, L, C), (0, 0, R, R))
    dyb = dyd.reshape(B, L, C)
    gw = torch.stack([(dyb * xp[:, j:j + L]).sum((0, 1)) for j in range(ks)], 1)
    gwa = torch.stack([(dyb * xp[:, j:j + L]).abs().sum((0, 1)) for j in range(ks)], 1)
    dw0, db0 = torch.randn(C, 1, ks, generator=g, device=device), torch.randn(C, generator=g, device=device)

    def launch():
        dx, dwt, db = Fenced(M, C, tt, device), Flat((C, 1, ks), device, dw0), Flat((C,), device, db0)
        det_run(device, c.det, [dwt.v, db.v], lambda: ops.dwconv_bwd(xin.v, w.v, dy.v, dx.v, dwt.v, db.v, B, L, ks))
        return dx, dwt, db
    dx, dwt, db = launch()
    dx.check(case, "dx")
    dwt.check(case, "dw")
    db.check(case, "db")
    check_frames(case, "dx", dx.v, ref_dx, OUT[T], sc_dx)
    # a thread adds its 64-frame run, the block meets in fixed point, then one atomic per block holding the channel
    runs = cdiv(L, DW_RUN_BWD)
    nb = B * cdiv((C // 8) * runs, 256)
    sb, fl = sum_bound(DW_RUN_BWD + 2, nb), fix_floor(B * runs + nb)
    check_elems(case, "dw", dwt.v.reshape(C, ks), dw0.double().reshape(C, ks) + gw, dw0.double().abs().reshape(C, ks) + gwa, sb, fl)
    check_elems(case, "db", db.v, db0.double() + dyd.sum(0), db0.double().abs() + dyd.abs().sum(0), sb, fl)
    if twice or c.det:
        r2 = launch()
        if c.det:
            assert all(torch.equal(bits(p.buf), bits(q.buf)) for p, q in zip((dx, dwt, db), r2)), f"{case}: two runs differ"


@dataclass(frozen=True)
class PI:
    T: str
    B: int
    L: int
    D: int
    E: int = 6
    bwd: bool = False
    det: bool = False

    @property
    def id(self):
        return f"proj_in{'_bwd' if self.bwd else ''}-{self.T}-E{self.E}{'-det' if self.det else ''}-{self.B}x{self.L}x{self.D}"

    def path(self, th=GPU_TH):
        return f"proj_in{'_bwd' if self.bwd else ''}/{self.T}"


def run_pi(c: PI, device, twice=False):
    T, B, L, D, E = c.T, c.B, c.L, c.D, c.E
    tt = TORCH[T]
    M = B * L
    g = _gen(device, 61)
    case = f"{c.id} [{c.path()}]"
    # xt rows of batch b scaled by 10^(b mod 3): a frame that reads another sequence's xt is off by a factor
    xt = Flat((B, E, L), device, torch.randn(B, E, L, generator=g, device=device) * (10.0 ** (torch.arange(B, device=device) % 3).float())[:, None, None])
    xf = xt.v.double().permute(0, 2, 1).reshape(M, E)
    if not c.bwd:
        W = Flat((D, E), device, 0.3 * torch.randn(D, E, generator=g, device=device))
        bias = Flat((D,), device, torch.randn(D, generator=g, device=device))
        x = Fenced(M, D, tt, device)
        ops.proj_in(xt.v, W.v, bias.v, x.v)
        x.check(case, "x")
        Wd = W.v.double()
        check_frames(case, "x", x.v, xf @ Wd.t() + bias.v.double(), OUT[T], xf.abs() @ Wd.abs().t() + bias.v.double().abs())
        return
    dx = Fenced(M, D, tt, device, torch.randn(M, D, generator=g, device=device))
    dxd = dx.v.double()
    dW0, db0 = torch.randn(D, E, generator=g, device=device), torch.randn(D, generator=g, device=device)

    def launch():
        dW, db = Flat((D, E), device, dW0), Flat((D,), device, db0)
        det_run(device, c.det, [dW.v, db.v], lambda: ops.proj_in_bwd(xt.v, dx.v, dW.v, db.v))
        return dW, db
    dW, db = launch()
    dW.check(case, "dW")
    db.check(case, "db")
    # od_proj_in_bwd: min(512, ceil(M / 64)) blocks; a wave strides over the frames (ceil(M / 4 blocks) each), 4 waves meet in LDS
    nb = min(512, max(1, cdiv(M, 64)))
    sb, fl = sum_bound(cdiv(M, 4 * nb) + 4, nb), fix_floor(nb) if c.det else 0.0
    check_elems(case, "dW", dW.v, dW0.double() + dxd.t() @ xf, dW0.double().abs() + dxd.abs().t() @ xf.abs(), sb, fl)
    check_elems(case, "db", db.v, db0.double() + dxd.sum(0), db0.double().abs() + dxd.abs().sum(0), sb, fl)
    if twice or c.det:
        r2 = launch()
        if c.det:
            assert all(torch.equal(bits(p.buf), bits(q.buf)) for p, q in zip((dW, db), r2)), f"{case}: two runs differ"


# ---------------------------------------------------------------- u-head (heads.hip)
@dataclass(frozen=True)
class UH:
    kind: str                 # fwd, fwd_varlen, bwd, tail, tail_varlen, tail_bwd
    B: int
    L: int
    U: int
    E: int = 6
    fam: str = "random"       # random / batch_distinct (xt of batch row b scaled by 3^(b mod 3))
    det: bool = False

    @property
    def id(self):
        return f"uhead_{self.kind}-{self.fam}-U{self.U}-E{self.E}{'-det' if self.det else ''}-{self.B}x{self.L}"

    def path(self, th=GPU_TH):
        return uhead_path(self.kind, self.B, self.L)


def uhead_path(kind, B, L):
    if kind in ("fwd", "fwd_varlen"):
        return f"uhead_{kind}/wpb{min(UWPB, max(1, cdiv(L, UOWN) * B // 512))}"
    return f"uhead_{kind}"


def uh_forward(x, P, m):
    """fp64 u_head (oracle u_head: dw3 -> 1x1 -> SiLU -> dw3 -> 1x1 -> SiLU) on (B, E, L), frames where m = 0 (past a sequence's end) being
    the zero padding of both convs.  Returns the intermediates."""
    def dw3(v, w, b):
        vp = torch.nn.functional.pad(v, (1, 1))
        L = v.shape[-1]
        return b[None, :, None] + sum(w[None, :, j, None] * vp[..., j:j + L] for j in range(3))
    z0 = dw3(x * m, P["w0"], P["b0"])
    z1 = torch.einsum("ce,bel->bcl", P["w1"], z0) + P["b1"][None, :, None]
    a1 = z1 * torch.sigmoid(z1) * m
    z3 = dw3(a1, P["w3"], P["b3"])
    z4 = torch.einsum("cd,bdl->bcl", P["w4"], z3) + P["b4"][None, :, None]
    return dict(x=x * m, z0=z0, z1=z1, a1=a1, z3=z3, z4=z4)


def silu_grad(z):
    s = torch.sigmoid(z)
    return s * (1 + z * (1 - s))


def uh_backward(F, P, dfm, L, A):
    """Gradients of sum_{b,c} dfm[b, c] / L sum_l silu(z4) with respect to the eight tensors; A = torch.abs gives, term by term, the sum of
    |products| along every path (the magnitude the fp32 sums carry), A = identity the gradient itself."""
    g4 = A(dfm)[:, :, None] / L * A(silu_grad(F["z4"]))
    G = {"b4": g4.sum((0, 2)), "w4": torch.einsum("bcl,bdl->cd", g4, A(F["z3"]))}
    dz3 = torch.einsum("cd,bcl->bdl", A(P["w4"]), g4)
    a1p = torch.nn.functional.pad(A(F["a1"]), (1, 1))
    L_ = dz3.shape[-1]
    G["b3"] = dz3.sum((0, 2))
    G["w3"] = torch.stack([(dz3 * a1p[..., j:j + L_]).sum((0, 2)) for j in range(3)], 1)
    dp = torch.nn.functional.pad(dz3, (1, 1))
    da1 = sum(A(P["w3"])[None, :, j, None] * dp[..., 2 - j:2 - j + L_] for j in range(3))
    dz1 = da1 * A(silu_grad(F["z1"]))
    G["b1"] = dz1.sum((0, 2))
    G["w1"] = torch.einsum("bcl,bel->ce", dz1, A(F["z0"]))
    dz0 = torch.einsum("ce,bcl->bel", A(P["w1"]), dz1)
    xp = torch.nn.functional.pad(A(F["x"]), (1, 1))
    G["b0"] = dz0.sum((0, 2))
    G["w0"] = torch.stack([(dz0 * xp[..., j:j + L_]).sum((0, 2)) for j in range(3)], 1)
    return G


UH_NAMES = ("w0", "b0", "w1", "b1", "w3", "b3", "w4", "b4")


def run_uhead(c: UH, device, twice=False):
    B, L, U, E = c.B, c.L, c.U, c.E
    g = _gen(device, 71)
    case = f"{c.id} [{c.path()}]"
    shapes = {"w0": (E, 1, 3), "b0": (E,), "w1": (U, E, 1), "b1": (U,), "w3": (U, 1, 3), "b3": (U,), "w4": (U, U, 1), "b4": (U,)}
    Pf = {n: Flat(s, device, (0.5 if n[0] == "w" else 0.3) * torch.randn(*s, generator=g, device=device)) for n, s in shapes.items()}
    P = {n: Pf[n].v.double().reshape(shapes[n][0], -1).squeeze(-1) if n[0] == "w" else Pf[n].v.double() for n in UH_NAMES}
    wl = [Pf[n].v for n in UH_NAMES]
    xt32 = torch.randn(B, E, L, generator=g, device=device)
    if c.fam == "batch_distinct":
        xt32 = xt32 * (3.0 ** (torch.arange(B, device=device) % 3).float())[:, None, None]
    xt = Flat((B, E, L), device, xt32)
    # sequence lengths: the varlen forms take L - 7 b (b odd) / L - b, one of them 1 when B > 2
    lens_l = [L] * B if not c.kind.endswith("varlen") else [max(1, L - 7 * b) if b % 2 else L - b for b in range(B)]
    if c.kind.endswith("varlen") and B > 2:
        lens_l[2] = 1
    lens = torch.tensor(lens_l, dtype=torch.int32, device=device)
    m = (torch.arange(L, device=device)[None, :] < lens.long()[:, None]).double()[:, None, :]
    # u-head chains (bounds): each z is a sum of up to U + 3 fp32 products, then SiLU (hardware exp, ~|z| 2^-24): measured against the
    # magnitudes the terms carry (A = abs in uh_backward; |z|-terms for the forward), (2U + 2E + 32) 2^-24 for the network, plus the sums
    net = 2 * U + 2 * E + 32
    nwin = cdiv(L, UOWN)
    if c.kind in ("fwd", "fwd_varlen", "bwd"):
        F = uh_forward(xt.v.double(), P, m)
    if c.kind in ("fwd", "fwd_varlen"):
        a4 = F["z4"] * torch.sigmoid(F["z4"]) * m
        ref_s = a4.sum(2)
        # forward magnitude: |a4| + |silu'(z4)| x (|b4| + |w4| (|b3| + |w3| |a1|)) per frame
        za3 = P["b3"].abs()[None, :, None] + sum(P["w3"].abs()[None, :, j, None] * torch.nn.functional.pad(F["a1"].abs(), (1, 1))[..., j:j + L]
                                                  for j in range(3))
        za4 = P["b4"].abs()[None, :, None] + torch.einsum("cd,bdl->bcl", P["w4"].abs(), za3)
        mag = ((a4.abs() + silu_grad(F["z4"]).abs() * za4) * m).sum(2)
        wpb = min(UWPB, max(1, nwin * B // 512))
        f0 = torch.randn(B, U, generator=g, device=device)

        def launch():
            fsum = Flat((B, U), device, f0)
            if c.kind == "fwd":
                det_run(device, c.det, [fsum.v], lambda: ops.uhead_fwd(xt.v, wl, fsum.v, U))
            else:
                det_run(device, c.det, [fsum.v], lambda: ops.uhead_fwd_varlen(xt.v, wl, fsum.v, lens, U))
            return fsum
        fsum = launch()
        fsum.check(case, "fsum")
        # a lane adds its wpb windows' frame, 32 lanes meet by shuffles, then one atomic per block (ceil(nwin / wpb) blocks per batch row)
        nb = cdiv(nwin, wpb)
        check_elems(case, "fsum", fsum.v, f0.double() + ref_s, f0.double().abs() + mag, net * 2.0 ** -24 + sum_bound(wpb + 5, nb),
                    fix_floor(nb) if c.det else 0.0)
        if twice or c.det:
            f2 = launch()
            if c.det:
                assert torch.equal(bits(f2.buf), bits(fsum.buf)), f"{case}: two runs differ"
        return
    if c.kind == "bwd":
        dfm = Flat((B, U), device, torch.randn(B, U, generator=g, device=device))
        ref = uh_backward(F, P, dfm.v.double(), L, lambda t: t)
        mag = uh_backward(F, P, dfm.v.double(), L, torch.abs)
        g0 = {n: torch.randn(*shapes[n], generator=g, device=device) for n in UH_NAMES}

        def launch():
            gr = {n: Flat(shapes[n], device, g0[n]) for n in UH_NAMES}
            det_run(device, c.det, [gr[n].v for n in UH_NAMES], lambda: ops.uhead_bwd(xt.v, wl, dfm.v, [gr[n].v for n in UH_NAMES], U))
            return gr
        gr = launch()
        # per block: 4 windows of 30 frames add serially into dw4 (120), the other sums meet by shuffles (5) and LDS atomics (4 windows);
        # ceil(nwin / 4) blocks per batch row, B rows
        nb = B * cdiv(nwin, UWPB)
        for n in UH_NAMES:
            gr[n].check(case, "d" + n)
            o = g0[n].double().reshape(ref[n].shape)
            check_elems(case, "d" + n, gr[n].v.reshape(ref[n].shape), o + ref[n], o.abs() + mag[n],
                        net * 2.0 ** -24 + sum_bound(UWPB * UOWN + 9, nb), fix_floor(nb) if c.det else 0.0)
        if twice or c.det:
            gr2 = launch()
            if c.det:
                assert all(torch.equal(bits(gr[n].buf), bits(gr2[n].buf)) for n in UH_NAMES), f"{case}: two runs differ"
        return
    # the tail: f = fsum / L (varlen: / lens[b]); fm = f (1 + mod[:U]) + mod[U:]; y = w . fm + b; u = u_scale softplus(y)
    US = 3.4641016
    fsum = Flat((B, U), device, 30.0 * torch.randn(B, U, generator=g, device=device))
    mod = Flat((B, 2 * U), device, 0.3 * torch.randn(B, 2 * U, generator=g, device=device))
    wo, bo = Flat((1, U), device, 0.3 * torch.randn(1, U, generator=g, device=device)), Flat((1,), device, torch.randn(1, generator=g, device=device))
    Ld = lens.double()[:, None] if c.kind == "tail_varlen" else float(L)
    f = fsum.v.double() / Ld
    sc, sh = mod.v.double()[:, :U], mod.v.double()[:, U:]
    fm = f * (1 + sc) + sh
    w_ = wo.v.double()[0]
    y = fm @ w_ + bo.v.double()
    yabs = (f.abs() * (1 + sc).abs() + sh.abs()) @ w_.abs() + bo.v.double().abs()
    sig = torch.sigmoid(y)
    tb = (U + 32) * 2.0 ** -24 + 2.0 ** -20          # the U-term dot, the division, exp / log1p (a few ulps)
    if c.kind in ("tail", "tail_varlen"):
        u = Flat((B,), device)
        if c.kind == "tail":
            ops.uhead_tail(fsum.v, mod.v, wo.v, bo.v, u.v, L, US)
        else:
            ops.uhead_tail_varlen(fsum.v, mod.v, wo.v, bo.v, u.v, lens, L, US)
        u.check(case, "u")
        check_elems(case, "u", u.v, US * torch.nn.functional.softplus(y), US * (torch.nn.functional.softplus(y) + sig * yabs), tb)
        return
    du = Flat((B,), device, torch.randn(B, generator=g, device=device))
    dy = du.v.double() * US * sig
    dyabs = du.v.double().abs() * US * (sig + sig * (1 - sig) * yabs)         # |dy| with the error of y carried through the sigmoid
    dw0_, db0_ = torch.randn(1, U, generator=g, device=device), torch.randn(1, generator=g, device=device)

    def launch():
        dfm, dmod = Flat((B, U), device), Flat((B, 2 * U), device)
        dwo, dbo = Flat((1, U), device, dw0_), Flat((1,), device, db0_)
        det_run(device, c.det, [dwo.v, dbo.v], lambda: ops.uhead_tail_bwd(fsum.v, mod.v, wo.v, bo.v, du.v, dfm.v, dmod.v, dwo.v, dbo.v, L, US))
        return dfm, dmod, dwo, dbo
    dfm, dmod, dwo, dbo = launch()
    for t, n in ((dfm, "dfm"), (dmod, "dmod"), (dwo, "dw_out"), (dbo, "db_out")):
        t.check(case, n)
    fma = f.abs() * (1 + sc).abs() + sh.abs()
    check_elems(case, "dfm", dfm.v, dy[:, None] * w_ * (1 + sc), dyabs[:, None] * w_.abs() * (1 + sc).abs(), tb)
    check_elems(case, "dmod", dmod.v, torch.cat([dy[:, None] * w_ * f, dy[:, None] * w_.expand(B, U)], 1),
                torch.cat([dyabs[:, None] * (w_ * f).abs(), dyabs[:, None] * w_.abs().expand(B, U)], 1), tb)
    # one atomic per batch row
    fl = fix_floor(B) if c.det else 0.0
    check_elems(case, "dw_out", dwo.v[0], dw0_.double()[0] + (dy[:, None] * fm).sum(0), dw0_.double()[0].abs() + (dyabs[:, None] * fma).sum(0),
                tb + sum_bound(0, B), fl)
    check_elems(case, "db_out", dbo.v, db0_.double() + dy.sum(), db0_.double().abs() + dyabs.sum(), tb + sum_bound(0, B), fl)
    if twice or c.det:
        r2 = launch()
        if c.det:
            assert all(torch.equal(bits(p.buf), bits(q.buf)) for p, q in zip((dfm, dmod, dwo, dbo), r2)), f"{case}: two runs differ"


RUN = {RC: run_row, SW: run_swiglu, FP: run_final, QK: run_qk, DW: run_dw, PI: run_pi, UH: run_uhead}


def run_case(c, device, twice=False):
    RUN[type(c)](c, device, twice)


# ---------------------------------------------------------------- the small cases (emulator and GPU)
# C: 8, 136, 504 (NCH 1), 520, 1024 (NCH 2), 1032, 1536 (NCH 3).  Backward lengths 67 / 130 / 200: 2 - 4 blocks of 64 frames per batch
# row, the last one ragged, and a last wave with 3 / 2 / 8 of its 16 rows.
# The forward families by C and cl (film and gate_film; gate takes the cl-none column): every family meets every cl mode, every NCH.
FWD_FAMS = {   # C: (cl none, cl per frame, cl broadcast)
    8: ("random", "eps", "batch_distinct"),
    136: ("row_scale", "batch_distinct", "eps"),
    504: ("eps", "random", "row_scale"),
    520: ("batch_distinct", "row_scale", "offset"),
    1024: ("offset", "eps", "random"),
    1032: ("random", "offset", "row_scale"),
    1536: ("row_scale", "random", "offset"),
}
SMALL = []
for T in TS:
    for C, fams in FWD_FAMS.items():
        for cl, fam in zip(("none", "frame", "bcast"), fams):
            SMALL += [RC("film", T, 3, 13, C, fam, cl), RC("gate_film", T, 3, 13, C, fam, cl)]
        SMALL.append(RC("gate", T, 3, 13, C, fams[0]))
    for kind in ("film_bwd", "gate_bwd"):
        for C, L, fam in ((8, 67, "random"), (136, 130, "row_scale"), (504, 200, "batch_distinct"), (520, 67, "eps"), (1032, 130, "offset"),
                          (1536, 67, "cancel"), (136, 200, "cancel"), (520, 130, "row_scale")):
            SMALL.append(RC(kind, T, 3, L, C, fam))
        SMALL += [RC(kind, T, 2, 130, 136, "random", det=True), RC(kind, T, 2, 67, 1032, "batch_distinct", det=True)]
    # the fused kernel: B ceil(L / 32) < 8 takes runs of 8 (emulator): (1, 100) 4 runs -> RUN 8, (3, 100) 12 -> RUN 32; lengths 100 and
    # 67 put the last run ragged, C 504 / 136 / 8
    for ks in (3, 5, 7, 9):
        SMALL += [RC("film_dwconv", T, 1, 100, 136, "random", ks=ks, h2=ks % 2 == 1), RC("film_dwconv", T, 3, 100, 504, "batch_distinct", ks=ks, h2=ks != 5),
                  RC("film_dwconv", T, 3, 67, 8, "eps", ks=ks, h2=ks == 5)]
    SMALL += [RC("film_dwconv", T, 1, 100, 136, "row_scale", ks=5, h2=False)]
    # SwiGLU: Hp 192 / 1024 / 1408 (NCH 1 / 2 / 3)
    for Hf, Hp in ((170, 192), (1000, 1024), (1365, 1408)):
        for fam in ("random", "row_scale", "silu_extreme", "eps"):
            SMALL += [SW(T, 21, Hf, Hp, fam), SW(T, 21, Hf, Hp, fam, bwd=True)]
        SMALL.append(SW(T, 21, Hf, Hp, "cancel", bwd=True))
    # final norm + projection: forward NCH 1 / 2, backward C <= 512, E 1 / 6 / 8
    SMALL += [FP(T, 3, 45, 504, 6, "row_scale"), FP(T, 3, 45, 1024, 8, "eps"), FP(T, 2, 45, 64, 1, "random"),
              FP(T, 3, 130, 504, 6, "random", bwd=True), FP(T, 3, 67, 136, 8, "row_scale", bwd=True), FP(T, 2, 130, 64, 1, "offset", bwd=True),
              FP(T, 2, 130, 504, 6, "batch_distinct", bwd=True, det=True), FP(T, 3, 130, 504, 6, "cancel", bwd=True),
              FP(T, 2, 67, 136, 8, "cancel", bwd=True)]
    # q/k: the position-major kernels at every (LPH, NIT) with B < 8 (bpw = B, lpw = 8 / B) and B >= 8 (bpw 8, a ragged last group);
    # the row kernel at hd 16 and at H hd / 8 not a multiple of 64
    for hd, Hs in ((32, (16, 32, 64)), (64, (8, 16, 32))):
        for j, H in enumerate(Hs):
            for bwd in (False, True):
                SMALL += [QK(T, 3, 11, H, hd, ("random", "row_scale", "eps")[j], 0.18 if j % 2 else 1.0, bwd),
                          QK(T, 11, 5, H, hd, ("batch_distinct", "random", "offset")[j], 1.0 if j % 2 else 0.18, bwd, det=bwd and j == 1)]
    for bwd in (False, True):
        SMALL += [QK(T, 2, 19, 3, 16, "random", 0.18, bwd), QK(T, 3, 9, 3, 64, "row_scale", 1.0, bwd), QK(T, 2, 19, 2, 32, "eps", 0.18, bwd, det=bwd)]
    SMALL += [QK(T, 3, 11, 16, 64, "cancel", 0.18, True), QK(T, 11, 5, 32, 32, "cancel", 1.0, True), QK(T, 2, 19, 3, 16, "cancel", 0.18, True)]
    # depthwise conv: small = B (C / 8) ceil(L / 32) < 10 takes runs of 4 (emulator): (1, 33, 16) is 4 threads -> RUN 4; (2, 97, 24) 24 ->
    # RUN 32 (frames 96, 97 past the third run border); the backward at L 129 / 65 (64-frame runs + 1), C / 8 = 3 and 65 (256 not a multiple)
    for ks in (3, 5, 7, 9):
        SMALL += [DW("dwconv", T, 1, 33, 16, ks), DW("dwconv", T, 2, 97, 24, ks, "batch_distinct"),
                  DW("dwconv_varlen", T, 1, 33, 16, ks), DW("dwconv_varlen", T, 3, 97, 24, ks, "batch_distinct"),
                  DW("dwconv_bwd", T, 3, 129, 24, ks, "batch_distinct"), DW("dwconv_bwd", T, 2, 65, 512 if ks > 5 else 1000, ks, det=ks == 5)]
    SMALL += [DW("dwconv_bwd", T, 2, 129, 520, 3, det=True)]
    SMALL += [PI(T, 3, 67, 520), PI(T, 2, 45, 1032, 8), PI(T, 3, 67, 520, bwd=True), PI(T, 2, 130, 1032, 1, bwd=True),
              PI(T, 2, 67, 136, 6, bwd=True, det=True)]
SMALL += [QK("f16", 2, 19, 3, 64, "random", 0.18), QK("f16", 3, 11, 16, 64, "row_scale", 1.0)]      # bf16 in, half out: always the row kernel
# u-head (fp32 only): L mod 30 in {29, 0, 1} (the last window ragged by one frame, full, one frame long), U 8 / 64; the backward at 2 - 8
# windows per batch row (one block of 4, or two with a ragged last block); the varlen forms with a sequence of length 1
SMALL += [UH("fwd", 2, 89, 64), UH("fwd", 3, 90, 8, fam="batch_distinct"), UH("fwd", 2, 121, 64, det=True), UH("fwd_varlen", 3, 121, 64, fam="batch_distinct"),
          UH("fwd_varlen", 2, 90, 8), UH("bwd", 2, 89, 64), UH("bwd", 3, 90, 8, fam="batch_distinct"), UH("bwd", 2, 151, 64, det=True),
          UH("bwd", 1, 240, 8), UH("tail", 5, 89, 64), UH("tail", 3, 90, 8), UH("tail_varlen", 5, 121, 64), UH("tail_bwd", 5, 89, 64),
          UH("tail_bwd", 3, 90, 8, det=True)]

# ---------------------------------------------------------------- GPU-only cases
# The bench shape (B 32 x L 8192, C 512 bf16: 128 backward blocks per batch row meet in the same atomics) for every backward with a
# cross-frame sum, launched twice with the deterministic shadow on (bit-identical); the sampler's 4 x 1115 for the forwards whose variant
# depends on size; RoPE positions up to 32767.
GPU_CASES = [
    RC("film_bwd", "bf16", 32, 8192, 512, det=True), RC("gate_bwd", "bf16", 32, 8192, 512, det=True),
    RC("film_bwd", "bf16", 32, 8192, 512, "offset"), RC("gate_bwd", "fp32", 8, 8192, 512, "row_scale", det=True),
    QK("bf16", 32, 8192, 16, 64, qs=0.18, bwd=True, det=True), QK("bf16", 1, 32767, 16, 64, "random", 0.18),
    QK("fp32", 1, 32767, 16, 64, "random", 1.0, bwd=True),
    DW("dwconv_bwd", "bf16", 32, 8192, 512, 5, det=True), DW("dwconv", "bf16", 32, 8192, 512, 5), DW("dwconv", "bf16", 4, 1115, 512, 5),
    SW("bf16", 32 * 8192, 1365, 1408, bwd=True), SW("bf16", 4 * 1115, 1365, 1408),
    FP("bf16", 32, 8192, 512, 6, bwd=True, det=True), FP("bf16", 4, 1115, 512, 6),
    PI("bf16", 32, 8192, 512, 6, bwd=True, det=True), PI("bf16", 4, 1115, 512, 6),
    RC("film_dwconv", "bf16", 32, 8192, 512, ks=5), RC("film_dwconv", "bf16", 4, 1115, 512, ks=5),
    RC("film", "bf16", 4, 1115, 512, cl="bcast"), RC("gate_film", "bf16", 4, 1115, 512), RC("gate", "bf16", 4, 1115, 512),
    QK("bf16", 4, 1115, 16, 64, qs=0.18),
]
# the conv kernels' RUN 32 at every (T, ks), at the GPU thresholds' edges: B ceil(L / 32) = 8 x 256 = 2048 runs (fused: RUN 32) against
# 8 x 255 (RUN 8); B (C / 8) ceil(L / 32) = 4 x 128 x 256 = 131072 threads (RUN 32) against 4 x 128 x 255 (RUN 4)
for T in TS:
    for ks in (3, 5, 7, 9):
        GPU_CASES += [RC("film_dwconv", T, 8, 8161, 136, "batch_distinct", ks=ks, h2=ks != 5), DW("dwconv", T, 4, 8161, 1024, ks, "batch_distinct"),
                      DW("dwconv_varlen", T, 4, 8161, 1024, ks, "batch_distinct")]
GPU_CASES += [RC("film_dwconv", "bf16", 8, 8160, 136, ks=5), DW("dwconv", "bf16", 4, 8160, 1024, 5)]
# the u-head forward at 1 - 4 windows per block (wpb = ceil(L / 30) B / 512, clamped): the sampler's 4 x 1115 (1), 4 x 7680 (1024 windows:
# 2), 6 x 7681 (1542: 3), the bench shape (4); the backward at the bench shape (U 64, E 6: 69 blocks per batch row meet in each gradient)
for k in ("fwd", "fwd_varlen"):
    GPU_CASES += [UH(k, 4, 1115, 64), UH(k, 4, 7680, 8), UH(k, 6, 7681, 64, fam="batch_distinct"), UH(k, 32, 8192, 64, det=k == "fwd")]
GPU_CASES += [UH("bwd", 32, 8192, 64, det=True), UH("bwd", 32, 8192, 64, fam="batch_distinct"), UH("tail_bwd", 32, 8192, 64, det=True)]


# ---------------------------------------------------------------- dispatch table
def _rows(cases, th):
    return {c.path(th) for c in cases}


def test_row_dispatch_table_matches_sources():
    """The thresholds and launcher conditions the path functions mirror are the ones in the sources; the cases of this file reach every
    row of the table on the GPU, and every row on the emulator."""
    row = open(os.path.join(CSRC, "rowops.hip")).read()
    misc = open(os.path.join(CSRC, "misc.hip")).read()
    heads = open(os.path.join(CSRC, "heads.hip")).read()
    emu = open(os.path.join(REPO, "tests", "emu", "build_emu.sh")).read()
    defs = {k: int(v) for k, v in re.findall(r"#define (OD_\w+) (\d+)", row + misc)}
    assert (defs["OD_FD_SMALL_RUNS"], defs["OD_DW_SMALL_THREADS"], defs["OD_QK_BPW"]) == (GPU_TH.fd_small, GPU_TH.dw_small, QK_BPW)
    flags = {k: int(v) for k, v in re.findall(r"-D(OD_\w+)=(\d+)", emu)}
    assert (flags["OD_FD_SMALL_RUNS"], flags["OD_DW_SMALL_THREADS"]) == (EMU_TH.fd_small, EMU_TH.dw_small)
    assert "OD_QK_BPW" not in flags
    for s in ("inline int nch_for(int C) { return (C + 511) / 512; }",
              f"constexpr int ROWS_PER_WAVE_BWD = {RPW_BWD};",
              "dim3 grid((L + 4 * ROWS_PER_WAVE_BWD - 1) / (4 * ROWS_PER_WAVE_BWD), B);",
              "const bool small = (long)B * ((L + 31) / 32) < OD_FD_SMALL_RUNS;",
              "const int run = small ? 8 : 32;",
              "if (C > 512 || (ksize != 3 && ksize != 5 && ksize != 7 && ksize != 9)) return OD_ERR_UNSUPPORTED;",
              "DISPATCH_T_NCH(dtype, nch_for(Hp),",
              "if (E > 8 || C > 1024) return OD_ERR_UNSUPPORTED;",
              "if (E > 8 || C > 512) return OD_ERR_UNSUPPORTED;",
              "if (dtype != OD_F16 && (lph == 4 || lph == 8) && (H * lph) % 64 == 0 && ldqkv >= 2 * H * hd) {",
              "if ((lph == 4 || lph == 8) && (H * lph) % 64 == 0) {",
              "if (nit == 2 || nit == 4 || nit == 8) {",
              "bpw = B < OD_QK_BPW ? B : OD_QK_BPW;",
              "lpw *= 4;"):
        assert s in row, s
    for s in (f"constexpr int DW_RUN_BWD = {DW_RUN_BWD};",
              "const bool small = (long)B * (C / 8) * ((L + 31) / 32) < OD_DW_SMALL_THREADS;",
              "const int run = small ? 4 : 32;",
              "if (C > 1024 || (ksize > 5 && C > 512)) return OD_ERR_UNSUPPORTED;",
              "if (E > 8) return OD_ERR_UNSUPPORTED;"):
        assert s in misc, s
    for s in (f"constexpr int UW = {UW};", f"constexpr int UOWN = {UOWN};", f"constexpr int UWPB = {UWPB};", "constexpr int MAXU = 64, MAXE = 8;",
              "const int nwin = (L + UOWN - 1) / UOWN;",
              "int wpb = (int)((long)nwin * B / 512);",
              "int wpb = (int)((long)nwin * B / 512);          // the same window split as od_uhead_fwd",
              "wpb = wpb < 1 ? 1 : (wpb > UWPB ? UWPB : wpb);",
              "dim3((nwin + wpb - 1) / wpb, B)",
              "OD_LAUNCH(uhead_bwd_kernel, dim3((nwin + UWPB - 1) / UWPB, B)",
              "for (int wi = 0; wi < UWPB; wi++) {",
              "if (U > MAXU || U % 8 || E > MAXE) return OD_ERR_UNSUPPORTED;"):
        assert s in heads, s
    assert UW == UOWN + 2          # a window is its owned frames and one halo frame either side
    assert len(set(ROWS)) == len(ROWS)
    gpu, emu_rows = _rows(SMALL + GPU_CASES, GPU_TH), _rows(SMALL, EMU_TH)
    assert gpu <= set(ROWS) and emu_rows <= set(ROWS), (gpu | emu_rows) - set(ROWS)
    assert set(ROWS) - gpu == set(), sorted(set(ROWS) - gpu)
    assert set(ROWS) - emu_rows == set(GPU_ONLY_ROWS), sorted(set(ROWS) - emu_rows)
    # the fused kernel with h2 written and NULL at both RUNs; the conv backward past 512 channels and with C / 8 not dividing 256
    for T in TS:
        for run in (8, 32):
            hs = {c.h2 for c in SMALL if isinstance(c, RC) and c.path(EMU_TH).startswith(f"film_dwconv/{T}/run{run}/")}
            assert hs == {True, False}, (T, run)
        assert {c.ks for c in SMALL if isinstance(c, DW) and c.kind == "dwconv_bwd" and c.T == T and c.C > 512} == {3, 5}
        assert any(isinstance(c, DW) and c.kind == "dwconv_bwd" and c.T == T and 256 % (c.C // 8) for c in SMALL)
    # every backward with a cross-frame sum has more than one block per batch row on the emulator, and meets the bench shape on the GPU
    assert all(c.L > 4 * RPW_BWD for c in SMALL if isinstance(c, RC) and c.kind.endswith("_bwd"))
    bench = {type(c).__name__ + getattr(c, "kind", "") for c in GPU_CASES if getattr(c, "B", 0) * getattr(c, "L", 0) == 32 * 8192 or
             getattr(c, "M", 0) == 32 * 8192}
    assert {"RCfilm_bwd", "RCgate_bwd", "QK", "DWdwconv_bwd", "SW", "FP", "PI", "RCfilm_dwconv", "UHfwd", "UHbwd"} <= bench, bench
    # the u-head: L mod 30 in {0, 1, 29} and U 8 / 64 for the forward and the backward on the emulator
    for k in ("fwd", "bwd"):
        cs = [c for c in SMALL if isinstance(c, UH) and c.kind == k]
        assert {c.L % UOWN for c in cs} >= {0, 1, UOWN - 1} and {c.U for c in cs} >= {8, 64}, k
    assert any(isinstance(c, UH) and c.kind == "bwd" and cdiv(c.L, UOWN) > UWPB for c in SMALL)
    # the GPU cases reach the large-size variants
    assert fd_path("bf16", 32, 8192, 5) == "film_dwconv/bf16/run32/ks5" and fd_path("bf16", 4, 1115, 5) == "film_dwconv/bf16/run8/ks5"
    assert dw_path("bf16", 32, 8192, 512, 5).split("/")[2] == "run32" and dw_path("bf16", 4, 1115, 512, 5).split("/")[2] == "run4"
    assert fd_path("fp32", 8, 8161, 3).split("/")[2] == "run32" and fd_path("bf16", 8, 8160, 5).split("/")[2] == "run8"
    assert dw_path("fp32", 4, 8161, 1024, 3).split("/")[2] == "run32" and dw_path("bf16", 4, 8160, 1024, 5).split("/")[2] == "run4"


SMALL_IDS = [c.id for c in SMALL]
assert len(set(SMALL_IDS)) == len(SMALL_IDS), "duplicate case ids"


@pytest.mark.parametrize("case", SMALL, ids=SMALL_IDS)
def test_row_path_small(dev, case):
    run_case(case, dev)


@pytest.fixture(scope="module")
def gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs the GPU")
    _lib._lib = None
    _lib.lib()
    return torch.device("cuda:0")


@pytest.mark.gpu
@pytest.mark.parametrize("case", GPU_CASES, ids=lambda c: c.id)
def test_row_path_large(gpu, case):
    run_case(case, gpu, twice=True)
    torch.cuda.empty_cache()
