"""Every attention kernel the library dispatches, against an fp64 reference computed from the same rounded operands, block by block
(64 query rows per (batch, head)), on inputs built to reach the branches where flash attention goes wrong.

Dispatch table (osu_dreamer_amd/csrc/attn.hip: launch_fwd, launch_bwd, od_flash_attn_*; osu_dreamer_amd/engine.py: Engine.fused_attn_bwd).
`fwd_path()` below mirrors those rules; `test_dispatch_table_matches_sources` re-reads the thresholds from the sources and checks that the
cases of this file still reach every row on both backends.

  path            operands   hd  q_prescaled  kernel                                       selected when                               e.g. (B, H, L)
  fwd16x/bf16     bf16       64  yes          flash_fwd16x_kernel<NWX, NQT, bf16_t>         L >= OD_FWD16X_MIN_L (2048; emulator: 128)  2 x 16 x 8192
  fwd16x/f16      f16        64  yes          flash_fwd16x_kernel<4, NQT, f16_t>            L >= OD_FWD16X_MIN_L                        2 x 16 x 8192
  fwd32/bf16      bf16       64  no / yes     flash_fwd32_kernel<NW, NQB, PRE>              not PRE, or L < OD_FWD16X_MIN_L             1 x 3 x 2047
  fwd32/f16       f16        64  no / yes     flash_fwd32_kernel<4, NQB, PRE, f16_t>        not PRE, or L < OD_FWD16X_MIN_L             1 x 3 x 2047
  generic/bf16    bf16       32  no           flash_fwd_kernel<bf16_t, 32, OD_ATTN_NW, PRE>  hd 32                                      1 x 3 x 2049
  fp32/hd64/q16   fp32       64  no / yes     flash_fwd_kernel<float, 64, 4, PRE, 1>        ceil(L / 128) B H < OD_FWD_NQT1_BELOW (2048) 1 x 3 x 2049
  fp32/hd64/q32   fp32       64  no           flash_fwd_kernel<float, 64, 4, PRE>           ceil(L / 128) B H >= OD_FWD_NQT1_BELOW       2 x 16 x 8192
  fp32/hd32       fp32       32  no           flash_fwd_kernel<float, 32, 4, PRE>           hd 32 (no 16-query form)                   1 x 3 x 2049
  x3p/hd64        fp32 (x3)  64  no           flash_fwd_x3p_kernel<4, PRE, OD_X3P_NQT>      OD_F32X3, hd 64                            1 x 3 x 8191
  x3/hd32         fp32 (x3)  32  no           flash_fwd_kernel<f32x3_t, 32, 4, PRE>         OD_F32X3, hd 32                            1 x 3 x 2049
  pair/bf16       bf16       64  no / yes     flash_bwd_dkv_kernel + flash_bwd_dq_kernel    Engine: L < 2048 (ops.flash_attn_bwd)      1 x 3 x 2047
  pair/fp32       fp32       64  no / yes     flash_bwd_dkv_kernel + flash_bwd_dq_kernel    Engine: fp32 compute, any L                1 x 3 x 2047
  fused/bf16      bf16       64  no / yes     fb kernel (attn_bwd_fused.hip)                Engine: L >= 2048 (ops.flash_attn_bwd_fused) 2 x 16 x 8192
  fused/f16       f16        64  no / yes     fb kernel, half operands                      Engine: attention in fp16, any L           2 x 16 x 8192

Layout as the engine uses it: q, k are column views of one [M, 2 dh] buffer, v of a [M, 3 dh] buffer; dq, dk are written into [M, 2 dh] and dv
into the last third of [M, 3 dh].  Every output is prefilled with NaN, so an element the kernel never writes fails the comparison.

Input families (built in fp32, rounded to the operand type; the reference reads the rounded operands back):
  random         N(0, 1).
  moving         the row maximum grows by >= 100 nats after the first key tile (a ramp along the keys): past fp32's e^88.7, so a lazy softmax
                 reference that does not move overflows instead of surviving by shift invariance.
  moving_last    the same jump, all of it in the last (ragged) key tile.
  padtrap        k = u + eps, q = -a u: every real score is about -40 nats.  A key past L that entered the softmax with score 0 would dominate.
  peaked         every query has one key >= 20 nats ahead of the rest, on tile borders (63 / 64, 191 / 192) and on key L - 1.
  peak_moderate  every query prefers key L - 1 by about 2.5 nats: counting that key twice (a padding row that repeats row L - 1) moves o visibly.
  offset         keys with a common component, |u| >= 8 |eps|: the partial sums of the fused kernel's dQ chain are much larger than dQ.
  heavy          (half operands) v x 300 and dO whose 64-row blocks span 1e-6 .. 1e-2: the amax pass and the power-of-two rescale into half.

Gradients are checked where the problem is well conditioned.  With a >= 20-nat peak, P_it = 1 - O(e^-20) and the true dS_it = P_it (dP_it - delta_i)
is O(e^-20), while any kernel forms dP_it - delta_i from a bf16 o: a 2^-9 |dO| |v| rounding of delta is the whole result — that is the problem, not
the kernel.  So `peaked` checks o, lse and dv (dv = P^T dO is well conditioned), and `moving_last` checks dq / dk only when the last tile holds
enough keys to share the probability.  The reference's delta uses the o the backward is handed, and where keys (queries) share a large
component (moving, offset, padtrap) dq and dk are measured against ls |dS| |K| (ls |dS|^T |Q|): see BOUNDS.
"""
import json
import math
import os
import re
from dataclasses import dataclass

import pytest
import torch

from osu_dreamer_amd import ops
from kernel_backend import REPO, block_rel_l2, dev  # noqa: F401

CSRC = os.path.join(REPO, "osu_dreamer_amd", "csrc")
OPS = {"bf16": torch.bfloat16, "f16": torch.float16, "fp32": torch.float32, "x3": torch.float32}
LN2 = math.log(2.0)
FB_KEYS = 192                 # keys per workgroup of the fused backward (attn_bwd_fused.hip: FB_KB = 4 * FB_NK * 16)
GPU_MIN_L, GPU_NQT1 = 2048, 2048    # attn.hip defaults, checked against the source below
EMU_MIN_L = 128               # tests/emu/build_emu.sh


def fwd_path(op, hd, pre, B, H, L, min_l=GPU_MIN_L, nqt1_below=GPU_NQT1):
    """The forward kernel launch_fwd picks (see the table above)."""
    if op == "f16":
        return "fwd16x/f16" if pre and L >= min_l else "fwd32/f16"
    if op == "bf16":
        if hd == 32:
            return "generic/bf16"
        return "fwd16x/bf16" if pre and L >= min_l else "fwd32/bf16"
    if op == "x3":
        return "x3p/hd64" if hd == 64 else "x3/hd32"
    if hd == 32:
        return "fp32/hd32"
    return "fp32/hd64/q16" if ((L + 127) // 128) * B * H < nqt1_below else "fp32/hd64/q32"


FWD_PATHS = ["fwd16x/bf16", "fwd16x/f16", "fwd32/bf16", "fwd32/f16", "generic/bf16", "fp32/hd64/q16", "fp32/hd64/q32", "fp32/hd32",
             "x3p/hd64", "x3/hd32"]
BWD_PATHS = ["pair/bf16", "pair/fp32", "fused/bf16", "fused/f16"]

# ---------------------------------------------------------------- bounds
# Relative L2 per 64-row block and over everything; lse as absolute nats per row.  bf16 output rounding alone is 2^-9 per element, about
# 2.3e-3 relative L2; half operands carry 3 more bits into P and dS, so what is left there is that same bf16 output rounding.
BOUNDS = {
    "bf16": dict(o=(8e-3, 4e-3), grad=(1.5e-2, 8e-3), lse=(1e-3, 2 ** -20), terms=(2 ** -8, 2 ** -9)),
    "f16": dict(o=(6e-3, 4e-3), grad=(1e-2, 8e-3), lse=(1e-3, 2 ** -20), terms=(2 ** -11, 2 ** -12)),
    "fp32": dict(o=(5e-5, 2e-5), grad=(5e-5, 2e-5), lse=(1e-5, 2 ** -20), terms=(2e-4, 1e-4)),
    "x3": dict(o=(1e-4, 5e-5), lse=(1e-5, 2 ** -16)),
}
# terms: dq and dk of the moving, offset and padtrap families, whose keys (queries) share a component larger than what varies: dq = ls sum_j dS_ij k_j
# cancels (sum_j dS_ij = 0), and every rounding of a term — dS to bf16 (2^-9) or half (2^-12) for the MFMA, a score to fp32 — is relative to
# |dS_ij| |k_j|, not to the result.  Those two are measured against the norms of ls |dS| |K| (ls |dS|^T |Q|): the bound is the operand's
# unit roundoff (fp32: the score's own rounding, 2^-24 mag, carried into P).  Measured on the emulator: bf16 1.2e-3, half 1.8e-4, fp32 4.5e-5.
# o, dv (dk) of fp32 / x3: the same score rounding moves the softmax weights; the bounds hold for mag <= 50 nats (x3, whose products carry
# 2^-16 instead of ~2^-21: 20 nats) and grow with it beyond (measured: x3 o 5.9e-5 at the padding trap's 40-nat scores, 2.8e-4 at 300;
# fp32 dv 2.8e-5 at 300).
# Half operands, dk and dv: P is stored as half, and a P below 2^-14 is subnormal with an absolute step of 2^-24, so key blocks whose whole
# weight is that small (the moving family at L = 8192: keys 12 nats below the row maximum) carry a relative error of 2^-25 / P.  Their
# denominator is at least 2^-12 of the largest block's (4.4e-2 measured against 1e-5 of it, one block of 4096 at 2 x 16 x 8192).
# lse: a + r mag nats per row.  A score is a sum of hd products, and its rounding is relative to mag = sum_d |q_d k_d| (in nats), not to the
# score: fp32 accumulation leaves ~sqrt(hd) 2^-24 mag (r = 2^-20 allows 16 ulp; 5.7e-5 nats measured where scores reach 200 nats), and the
# fp32-as-3-x-bf16 product drops lo x lo and rounds lo, 2^-16 of each product (r = 2^-16; 7.9e-4 nats measured at 200-nat scores, head_dim 32).


def _report(case, name, blk, glob, bound):
    path = os.environ.get("OD_ATTN_PATHS_REPORT")
    if path:
        with open(path, "a") as f:
            f.write(json.dumps(dict(case=case, what=name, block=blk, glob=glob, bound=bound)) + "\n")


def check_blocks(case, name, out, ref, bound, scale=None, floor_max=1e-5):
    blk, glob, where = block_rel_l2(out, ref, scale=scale, floor_max=floor_max)
    _report(case, name, blk, glob, bound)
    assert blk <= bound[0] and glob <= bound[1], f"{case} {name}: block {blk:.3e} at (head, block) {where}, global {glob:.3e}, bounds {bound}"


def check_lse(case, lse, ref, mag, bound):
    """Per row: |lse - lse_ref| <= a + r mag, mag = the row's largest sum_d |q_d k_d| in nats (bound = (a, r))."""
    err = (lse.double() - ref).abs()
    worst = float((err / (bound[0] + bound[1] * mag)).max())
    _report(case, "lse", float(err.max()), worst, bound)
    assert worst <= 1.0, f"{case} lse: {float(err.max()):.3e} nats, {worst:.2f} x the bound {bound}"


# ---------------------------------------------------------------- input families (logit space: logits = scale q . k)
def make_inputs(fam, B, H, L, hd, device, seed=0):
    g = torch.Generator(device=device).manual_seed(seed)
    shape = (B, H, L, hd)

    def rn(*s):
        return torch.randn(*s, generator=g, device=device)
    scale = 1 / math.sqrt(hd)
    q, k, v, do = rn(*shape), rn(*shape), rn(*shape), rn(*shape)
    if fam in ("moving", "moving_last"):
        w = rn(B, H, 1, hd)
        w = w / w.norm(dim=-1, keepdim=True)
        q = q - (q * w).sum(-1, keepdim=True) * w + w / scale           # logits = gamma_j + (noise of ~1 nat)
        j = torch.arange(L, device=device, dtype=torch.float32)
        if fam == "moving":
            gamma = 200.0 * j / (L - 1)
        else:
            gamma = torch.where(j >= 64 * ((L - 1) // 64), 150.0, 0.0)
        k = k + gamma[:, None] * w
    elif fam == "padtrap":
        u = rn(B, H, 1, hd)
        a = 40.0 / (scale * u.pow(2).sum(-1, keepdim=True))
        k = u + 0.3 * k
        q = -a * u + 0.3 * q
    elif fam in ("peaked", "peak_moderate"):
        T = [L - 1] if fam == "peak_moderate" else sorted({t for t in (63, 64, 191, 192, L - 1) if t < L})
        n = len(T)
        GR = (2.5 if fam == "peak_moderate" else 26.0) / scale
        q = 0.5 * q
        q[..., :n] = 0
        k[..., :n] = 0
        for m, t in enumerate(T):
            k[:, :, t, :] = 0
            k[:, :, t, m] = math.sqrt(GR)
        target = torch.arange(L, device=device) % n
        target[L - 1] = n - 1                                           # row L - 1 peaks on key L - 1
        q.scatter_(-1, target.view(1, 1, L, 1).expand(B, H, L, 1), math.sqrt(GR))
    elif fam == "offset":
        u = rn(B, H, 1, hd)
        eps = 0.05 * k
        assert float(u.norm(dim=-1).min()) >= 8 * float(eps.norm(dim=-1).max()), "keys need a dominant common component"
        k = u + eps
        q = 4.0 * q
    elif fam == "heavy":
        v = 300.0 * v
        nb = (L + 63) // 64
        r = torch.rand(B, H, nb, generator=g, device=device)
        r.view(-1)[0], r.view(-1)[-1] = 0.0, 1.0
        do = do * (10.0 ** (-6.0 + 4.0 * r)).repeat_interleave(64, -1)[..., :L, None]
    else:
        assert fam == "random", fam
    return q, k, v, do


def layout(x):                    # (B, H, L, hd) -> [B L, H hd]
    B, H, L, hd = x.shape
    return x.permute(0, 2, 1, 3).reshape(B * L, H * hd)


def heads(x, B, H, L, hd):        # [B L, H hd] -> (B, H, L, hd)
    return x.reshape(B, L, H, hd).permute(0, 2, 1, 3)


# ---------------------------------------------------------------- fp64 reference, one (batch, head) at a time, chunked over queries
def reference(q, k, v, do, ls, grads, o_given=None):
    """q, k, v, do: (L, hd) float64; logits = ls q k^T.  Returns o, lse and (grads) dq, dk, dv, plus what the fixtures assert about the
    scores: the smallest growth of the row maximum after the first 64 keys, the smallest gap between a row's two largest scores, and per
    row the largest ls sum_d |q_d k_d| (the magnitude the score's own rounding is relative to).
    `o_given`: the o the backward is handed (the forward's stored output), for delta = rowsum(dO o) as the kernels form it — the rounding of o
    to its storage type is the forward's error, checked there; through delta it reaches dq as ls delta_err sum_j P_ij k_j, which keys with a
    large common component (the moving and offset families) amplify far beyond what the backward itself contributes."""
    L = q.shape[0]
    chunk = max(64, min(L, (1 << 26) // L))
    o, lse = torch.empty_like(q), q.new_empty(L)
    dq, dk, dv, dqm, dkm = torch.empty_like(q), torch.zeros_like(k), torch.zeros_like(v), torch.empty_like(q), torch.zeros_like(k)
    growth, gap = math.inf, math.inf
    mag = q.new_empty(L)
    for c0 in range(0, L, chunk):
        c1 = min(L, c0 + chunk)
        s = ls * (q[c0:c1] @ k.t())
        if L > 64:
            growth = min(growth, float((s[:, 64:].amax(-1) - s[:, :64].amax(-1)).min()))
        mag[c0:c1] = ls * (q[c0:c1].abs() @ k.abs().t()).amax(-1)
        top = s.topk(2, -1).values
        gap = min(gap, float((top[:, 0] - top[:, 1]).min()))
        m = s.amax(-1, keepdim=True)
        p = torch.exp(s - m)
        lsum = p.sum(-1, keepdim=True)
        p /= lsum
        lse[c0:c1] = (m + lsum.log()).squeeze(-1)
        oc = p @ v
        o[c0:c1] = oc
        if grads:
            dc = do[c0:c1]
            og = oc if o_given is None else o_given[c0:c1]
            ds = p * (dc @ v.t() - (dc * og).sum(-1, keepdim=True))
            dq[c0:c1] = ls * (ds @ k)
            dqm[c0:c1] = ls * (ds.abs() @ k.abs())
            dk += ls * (ds.t() @ q[c0:c1])
            dkm += ls * (ds.abs().t() @ q[c0:c1].abs())
            dv += p.t() @ dc
        del s, p
    return dict(o=o, lse=lse, dq=dq, dk=dk, dv=dv, dq_terms=dqm, dk_terms=dkm, growth=growth, gap=gap, mag=mag)


def checked_heads(B, H, L):
    """Every (batch, head) up to L = 8192; at longer lengths the first and the last."""
    if L <= 8192:
        return [(b, h) for b in range(B) for h in range(H)]
    return [(0, 0), (B - 1, H - 1)]


@dataclass
class Case:
    op: str           # operand type: bf16, f16, fp32, x3
    hd: int
    pre: bool
    fam: str
    B: int
    H: int
    L: int
    bwd: str = ""     # "", "pair", "fused"

    @property
    def id(self):
        return f"{self.bwd or 'fwd'}-{self.op}-hd{self.hd}-{'pre' if self.pre else 'raw'}-{self.fam}-{self.B}x{self.H}x{self.L}"


def grads_conditioned(fam, L):
    if fam == "peaked":
        return False
    if fam == "moving_last":
        return L % 64 == 0 or L % 64 >= 16
    return True


def run_case(c: Case, device):
    B, H, L, hd = c.B, c.H, c.L, c.hd
    M, dh = B * L, H * hd
    scale = 1 / math.sqrt(hd)
    cq = scale * math.log2(math.e)
    top = OPS[c.op]
    obf = torch.bfloat16 if c.op == "f16" else top                       # half operands: o, dO and the gradients are bf16
    Q, K, V, dO = make_inputs(c.fam, B, H, L, hd, device)
    if c.pre:
        Q = Q * cq                                                        # q' = q scale log2(e): logits ln2 q' . k
    qk = torch.empty(M, 2 * dh, dtype=top, device=device)
    qkv = torch.full((M, 3 * dh), float("nan"), dtype=top, device=device)
    qk[:, :dh], qk[:, dh:], qkv[:, 2 * dh:] = layout(Q).to(top), layout(K).to(top), layout(V).to(top)
    q, k, v = qk[:, :dh], qk[:, dh:], qkv[:, 2 * dh:]
    o = torch.full((M, dh), float("nan"), dtype=obf, device=device)
    lse = torch.full((B, H, L), float("nan"), device=device)
    ops.flash_attn_fwd(q, k, v, o, lse, B, H, L, hd, scale, x3=c.op == "x3", q_prescaled=c.pre)
    grads = bool(c.bwd)
    if grads:
        do = layout(dO).to(obf)
        dqk = torch.full((M, 2 * dh), float("nan"), dtype=obf, device=device)
        dqkv = torch.full((M, 3 * dh), float("nan"), dtype=obf, device=device)
        dq, dk, dv = dqk[:, :dh], dqk[:, dh:], dqkv[:, 2 * dh:]
        if c.bwd == "pair":
            delta = torch.full((B, H, L), float("nan"), device=device)
            ops.flash_attn_bwd(q, k, v, o, do, lse, delta, dq, dk, dv, B, H, L, hd, scale, q_prescaled=c.pre)
        else:
            ws = ops.FusedAttnBwdWorkspace(B, H, L, device, top)
            ops.flash_attn_bwd_fused(q, k, v, o, do, lse, dq, dk, dv, B, H, L, hd, scale, ws, q_prescaled=c.pre)
            assert ws.status() == 0
        assert bool(torch.isnan(dqkv[:, :2 * dh]).all()), "the backward wrote outside dv's columns"
    ls = LN2 if c.pre else scale
    sel = checked_heads(B, H, L)
    hq, hk, hv = (heads(t, B, H, L, hd) for t in (q, k, v))
    outs = {"o": heads(o, B, H, L, hd)}
    if grads:
        hdo = heads(do, B, H, L, hd)
        outs.update(dq=heads(dq, B, H, L, hd), dk=heads(dk, B, H, L, hd), dv=heads(dv, B, H, L, hd))
    refs = {n: [] for n in list(outs) + ["lse", "mag"] + (["dq_terms", "dk_terms"] if grads else [])}
    for b, h in sel:
        r = reference(hq[b, h].double(), hk[b, h].double(), hv[b, h].double(), hdo[b, h].double() if grads else None, ls, grads,
                      outs["o"][b, h].double() if grads else None)
        if c.fam in ("moving", "moving_last"):
            assert r["growth"] >= 100, f"the fixture must move the row maximum by >= 100 nats after the first tile ({r['growth']:.1f})"
        if c.fam == "peaked":
            assert r["gap"] >= 20, f"the fixture must give every row a >= 20-nat peak ({r['gap']:.1f})"
        for n in refs:
            refs[n].append(r[n])
    bnd = BOUNDS[c.op]
    idx = torch.tensor([b * H + h for b, h in sel], device=device)
    pick = lambda t: t.reshape(B * H, *t.shape[2:])[idx]                # noqa: E731
    check_lse(c.id, pick(lse), torch.stack(refs["lse"]), torch.stack(refs["mag"]), bnd["lse"])
    mag = float(torch.stack(refs["mag"]).max())
    grow = max(1.0, mag / {"fp32": 50, "x3": 20}.get(c.op, math.inf))
    check_blocks(c.id, "o", pick(outs["o"]), torch.stack(refs["o"]), [b * grow for b in bnd["o"]])
    if grads:
        names = ("dq", "dk", "dv") if grads_conditioned(c.fam, L) else ("dv",)
        for n in names:
            if n in ("dq", "dk") and c.fam in ("moving", "offset", "padtrap"):
                check_blocks(c.id, n + "/terms", pick(outs[n]), torch.stack(refs[n]), bnd["terms"], scale=torch.stack(refs[n + "_terms"]))
            else:
                check_blocks(c.id, n, pick(outs[n]), torch.stack(refs[n]), [b * grow for b in bnd["grad"]],
                             floor_max=2 ** -12 if c.op == "f16" and n != "dq" else 1e-5)


# ---------------------------------------------------------------- the cases
FWD_CONFIGS = [("bf16", 64, True), ("bf16", 64, False), ("f16", 64, True), ("f16", 64, False), ("bf16", 32, False), ("fp32", 64, False),
               ("fp32", 64, True), ("fp32", 32, False), ("x3", 64, False), ("x3", 32, False)]
# small shapes: through the `dev` fixture, so they run on the emulator (where fwd16x starts at L = 128) and on the GPU
SMALL_FWD = {"random": [(2, 1, 193)], "moving": [(1, 1, 300)], "moving_last": [(1, 1, 300)], "padtrap": [(1, 1, 193), (1, 1, 319)],
             "peaked": [(1, 2, 257)], "peak_moderate": [(1, 1, 257)]}
SMALL_CASES = [Case(op, hd, pre, fam, *s) for op, hd, pre in FWD_CONFIGS for fam, shapes in SMALL_FWD.items() for s in shapes]
SMALL_CASES += [Case(op, 64, True, fam, 1, 1, L) for op in ("bf16", "f16") for fam, L in (("random", 127), ("padtrap", 127), ("padtrap", 65))]
SMALL_CASES += [Case("f16", 64, pre, "heavy", 1, 1, 300) for pre in (False, True)]
SMALL_BWD = [("random", (1, 2, 193)), ("moving", (1, 1, 300)), ("padtrap", (1, 1, 193)), ("peak_moderate", (1, 1, 257)), ("peaked", (1, 1, 257)),
             ("offset", (1, 1, 450))]
SMALL_CASES += [Case(op, 64, pre, fam, *s, bwd=kind) for kind, op in (("pair", "bf16"), ("pair", "fp32"), ("fused", "bf16"), ("fused", "f16"))
                for pre in (False, True) for fam, s in (SMALL_BWD if pre else SMALL_BWD[:3])]
SMALL_CASES += [Case("f16", 64, pre, "heavy", 1, 1, 300, bwd="fused") for pre in (False, True)]
SMALL_CASES += [Case("bf16", 64, True, "padtrap", 1, 1, 127, bwd="pair"), Case("bf16", 64, True, "random", 1, 11, 193, bwd="fused")]

# the long lengths: 2047 / 2048 / 2049 around the fwd16x and fused switches, 8191 / 8192, 32768 (BASELINE configs[4]); B H not a multiple of
# 8 (ragged XCD queues of the fused kernel) and 3 x 13 = 39 > 8 x FB_SLOTS (32) (batch, head) pairs
LONG_CASES = []
for op in ("bf16", "f16"):
    LONG_CASES += [Case(op, 64, True, fam, 2, 16, 8192) for fam in ("random", "moving", "peaked")]
    LONG_CASES += [Case(op, 64, True, fam, 1, 3, 2049) for fam in ("padtrap", "moving_last")]
    LONG_CASES += [Case(op, 64, True, "random", 1, 3, 2048), Case(op, 64, True, "padtrap", 2, 3, 8191),
                   Case(op, 64, True, "peak_moderate", 2, 3, 8191), Case(op, 64, True, "moving", 1, 2, 32768)]
    LONG_CASES += [Case(op, 64, True, fam, 1, 3, 2047) for fam in ("random", "padtrap", "moving_last")]
    LONG_CASES += [Case(op, 64, False, fam, 1, 3, 8191) for fam in ("moving", "padtrap")]
LONG_CASES += [Case("f16", 64, True, "heavy", 2, 16, 8192)]
LONG_CASES += [Case("fp32", 64, False, fam, 2, 16, 8192) for fam in ("random", "moving", "peaked")]
LONG_CASES += [Case("fp32", 64, False, "padtrap", 2, 16, 8191), Case("fp32", 64, True, "moving", 1, 3, 2049)]
LONG_CASES += [Case("x3", 64, False, fam, 1, 3, 8191) for fam in ("random", "moving", "padtrap")]
LONG_CASES += [Case(op, 32, False, fam, 1, 3, 2049) for op in ("bf16", "fp32", "x3") for fam in ("random", "padtrap", "peak_moderate", "moving")]
for op in ("bf16", "f16"):
    LONG_CASES += [Case(op, 64, True, fam, 2, 16, 8192, bwd="fused") for fam in ("random", "moving", "peak_moderate")]
    LONG_CASES += [Case(op, 64, True, "padtrap", 3, 13, 2049, bwd="fused"), Case(op, 64, True, "offset", 2, 3, 8191, bwd="fused"),
                   Case(op, 64, False, "random", 1, 3, 2049, bwd="fused"), Case(op, 64, False, "padtrap", 1, 3, 2048, bwd="fused")]
LONG_CASES += [Case("f16", 64, True, "heavy", 2, 16, 8192, bwd="fused"), Case("f16", 64, True, "heavy", 1, 2, 32768, bwd="fused"),
               Case("bf16", 64, True, "random", 1, 2, 32768, bwd="fused")]
LONG_CASES += [Case(op, 64, pre, fam, 1, 3, 2047, bwd="pair") for op in ("bf16", "fp32") for pre in (False, True)
               for fam in ("random", "padtrap", "moving")]


def _emu_path(c):
    return fwd_path(c.op, c.hd, c.pre, c.B, c.H, c.L, min_l=EMU_MIN_L)


def _gpu_path(c):
    return fwd_path(c.op, c.hd, c.pre, c.B, c.H, c.L)


def _bwd_path(c):
    return f"{c.bwd}/{'fp32' if c.op == 'fp32' else c.op}"


def test_dispatch_table_matches_sources():
    """The thresholds `fwd_path` uses are the ones in the sources, and the cases of this file reach every path of the table: on the GPU
    with every input family, on the emulator with the small ones (the 32-query fp32 form needs >= 2048 workgroups: GPU only)."""
    src = open(os.path.join(CSRC, "attn.hip")).read()
    assert int(re.search(r"#define OD_FWD16X_MIN_L (\d+)", src).group(1)) == GPU_MIN_L
    assert int(re.search(r"#define OD_FWD_NQT1_BELOW (\d+)", src).group(1)) == GPU_NQT1
    assert "blocks2 = ((L + NW * 32 - 1) / (NW * 32)) * B * H" in src and "constexpr int NW = Stage<T, HD>::TR ? OD_ATTN_NW : 4;" in src
    assert "if (PRE && L >= fwd16x_min_l_h)" in src and "HD == 64 && PRE && L >= fwd16x_min_l)" in src
    assert re.search(r"-DOD_FWD16X_MIN_L=(\d+)", open(os.path.join(REPO, "tests", "emu", "build_emu.sh")).read()).group(1) == str(EMU_MIN_L)
    fsrc = open(os.path.join(CSRC, "attn_bwd_fused.hip")).read()
    assert "constexpr int FB_NK = 3;" in fsrc and "FB_KB = 4 * FB_NK * 16;" in fsrc
    eng = open(os.path.join(REPO, "osu_dreamer_amd", "engine.py")).read()
    fused_min = int(re.search(r"return self\.L >= (\d+)", eng).group(1))
    assert fused_min == 2048
    # every forward path, on the GPU: with every family it is meant to face
    fwd_fams = {"random", "moving", "padtrap"}
    for p in FWD_PATHS:
        seen = {c.fam for c in LONG_CASES + SMALL_CASES if _gpu_path(c) == p}
        assert fwd_fams <= seen, (p, seen)
        assert any(_emu_path(c) == p for c in SMALL_CASES) or p == "fp32/hd64/q32", p
    for p in ("fwd16x/bf16", "fwd16x/f16"):
        assert {c.L for c in LONG_CASES if _gpu_path(c) == p} >= {2048, 2049, 8191, 8192, 32768}
        assert {"moving_last", "peaked", "peak_moderate"} <= {c.fam for c in LONG_CASES if _gpu_path(c) == p}
    assert {c.L for c in LONG_CASES if _gpu_path(c) in ("fwd32/bf16", "fwd32/f16") and c.pre} == {2047}
    # ragged lengths of the padding trap: L mod 64 in {1, 63}, and a ragged 192-key block of the fused kernel
    trap = [c for c in SMALL_CASES + LONG_CASES if c.fam == "padtrap"]
    assert {c.L % 64 for c in trap} >= {1, 63} and any(c.L % FB_KEYS not in (0,) for c in trap if c.bwd == "fused")
    # every backward path, as the engine would pick it (fused from L = 2048 in bf16; half operands: fused only)
    for p in BWD_PATHS:
        assert any(_bwd_path(c) == p for c in LONG_CASES) and any(_bwd_path(c) == p for c in SMALL_CASES), p
    for c in LONG_CASES:
        if c.bwd == "fused" and c.op == "bf16":
            assert c.L >= fused_min, c.id
        if c.bwd == "pair" and c.op == "bf16":
            assert c.L < fused_min, c.id
    assert any(c.bwd == "fused" and c.B * c.H > 32 and (c.B * c.H) % 8 for c in LONG_CASES)


@pytest.mark.parametrize("case", SMALL_CASES, ids=lambda c: c.id)
def test_attention_path_small(dev, case):
    run_case(case, dev)


@pytest.fixture(scope="module")
def gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs the GPU")
    from osu_dreamer_amd import _lib
    _lib._lib = None
    _lib.lib()
    return torch.device("cuda:0")


@pytest.mark.gpu
@pytest.mark.parametrize("case", LONG_CASES, ids=lambda c: c.id)
def test_attention_path_long(gpu, case):
    run_case(case, gpu)


@pytest.mark.gpu
@pytest.mark.parametrize("fam", ["random", "offset"])
@pytest.mark.parametrize("B,H", [(1, 2), (1, 8)])
def test_fused_dq_chain_171_hops(gpu, fam, B, H):
    """The fused backward's packed dQ chain over the 171 key blocks of L = 32768 (FB_PACK: the running dQ re-rounded to 13 mantissa bits at
    every hop, relative to the running partial sum): its dq against fp64, next to the two-kernel pair's dq (summed in registers), on random
    keys and on keys with a common component (partial sums much larger than dQ, since the sum of dS over the keys is 0).  (1, 2): both
    (batch, head)s; (1, 8): the last one.  Bound: both are dominated by the bf16 dS the MFMAs read and the bf16 dq they write; the chain's
    share is <= 171 x 2^-14 of the largest partial sum in the worst case, ~sqrt(171 / 6) x 2^-14 / sqrt(3) of it as a random walk."""
    from kernel_backend import block_errors
    L, hd = 32768, 64
    M, dh = B * L, H * hd
    scale = 1 / math.sqrt(hd)
    bf = torch.bfloat16
    Q, K, V, dO = make_inputs(fam, B, H, L, hd, gpu, seed=3)
    qk = torch.empty(M, 2 * dh, dtype=bf, device=gpu)
    qkv = torch.empty(M, 3 * dh, dtype=bf, device=gpu)
    qk[:, :dh], qk[:, dh:], qkv[:, 2 * dh:] = layout(Q * scale * math.log2(math.e)).to(bf), layout(K).to(bf), layout(V).to(bf)
    q, k, v = qk[:, :dh], qk[:, dh:], qkv[:, 2 * dh:]
    do = layout(dO).to(bf)
    o = torch.empty(M, dh, dtype=bf, device=gpu)
    lse = torch.empty(B, H, L, device=gpu)
    ops.flash_attn_fwd(q, k, v, o, lse, B, H, L, hd, scale, q_prescaled=True)
    dqf, dqp = (torch.full((M, 2 * dh), float("nan"), dtype=bf, device=gpu) for _ in range(2))
    dvf = torch.full((M, 3 * dh), float("nan"), dtype=bf, device=gpu)
    ws = ops.FusedAttnBwdWorkspace(B, H, L, gpu)
    ops.flash_attn_bwd_fused(q, k, v, o, do, lse, dqf[:, :dh], dqf[:, dh:], dvf[:, 2 * dh:], B, H, L, hd, scale, ws, q_prescaled=True)
    assert ws.status() == 0
    delta = torch.empty(B, H, L, device=gpu)
    dvp = torch.full((M, 3 * dh), float("nan"), dtype=bf, device=gpu)
    ops.flash_attn_bwd(q, k, v, o, do, lse, delta, dqp[:, :dh], dqp[:, dh:], dvp[:, 2 * dh:], B, H, L, hd, scale, q_prescaled=True)
    sel = [(0, 0), (0, 1)] if H == 2 else [(B - 1, H - 1)]
    hq, hk, hv, hdo = (heads(t, B, H, L, hd) for t in (q, k, v, do))
    hf, hp = heads(dqf[:, :dh], B, H, L, hd), heads(dqp[:, :dh], B, H, L, hd)
    ref = torch.stack([reference(hq[b, h].double(), hk[b, h].double(), hv[b, h].double(), hdo[b, h].double(), LN2, True)["dq"] for b, h in sel])
    fused = torch.stack([hf[b, h] for b, h in sel])
    pair = torch.stack([hp[b, h] for b, h in sel])
    ef, gf = block_errors(fused, ref)
    ep, gp = block_errors(pair, ref)
    case = f"chain-{fam}-{B}x{H}x{L}"
    _report(case, "dq fused", float(ef.max()), gf, None)
    _report(case, "dq pair", float(ep.max()), gp, None)
    assert gf <= 1.25 * gp, f"{case}: fused dq {gf:.3e} against the pair's {gp:.3e} (global)"
    bad = ef > 1.5 * ep + 1e-4
    assert not bool(bad.any()), f"{case}: {int(bad.sum())} blocks, worst fused {float(ef.max()):.3e} against pair {float(ep.max()):.3e}"
