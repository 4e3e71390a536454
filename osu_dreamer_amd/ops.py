"""Thin torch-tensor front end over the C ABI (include/osu_dreamer_hip.h).

Each function forwards raw pointers/sizes to one `od_*` entry point on the current HIP
stream.  Tensors are only storage here: no arithmetic is done with torch ops.
Activations are frame-major 2-D tensors [M = B*L, C] (see csrc/od_common.h).
"""
from __future__ import annotations

import os
from typing import Optional

import torch

from . import _lib
from ._lib import OD_ACT_NONE, OD_ACT_SILU, OD_BF16, OD_EPI_NONE, OD_EPI_SILU, OD_F32, OD_F32X3, OD_F32X3W


def dt_code(dtype: torch.dtype) -> int:
    if dtype == torch.float32:
        return OD_F32
    if dtype == torch.bfloat16:
        return OD_BF16
    if dtype == torch.float16:          # the operand type of the attention core when the host asks for "attention in fp16" (nothing else takes it)
        return _lib.OD_F16
    raise TypeError(f"unsupported compute dtype {dtype}")


class SplitWeight:
    """A GEMM weight packed by `pack_weight(..., split=True)`: fp32-sized storage holding, per row and per 32-element K slab, the 32 bf16
    high halves then the 32 low halves (OD_F32X3W).  Only the fp32-as-3-x-bf16 GEMMs read it."""

    def __init__(self, storage: torch.Tensor):
        self.t = storage


def mm_code(dtype: torch.dtype, x3: bool, w=None) -> int:
    """Compute-type code of a matrix product: fp32 tensors run as three bf16 MFMAs per product when `x3` (OD_F32X3; OD_F32X3W when
    the weight was pre-split at pack time)."""
    if isinstance(w, SplitWeight):
        if not (x3 and dtype == torch.float32):
            raise ValueError("a pre-split weight can only feed the fp32-as-3-x-bf16 product")
        return OD_F32X3W
    return OD_F32X3 if (x3 and dtype == torch.float32) else dt_code(dtype)


def _w(W):
    return W.t if isinstance(W, SplitWeight) else W


def _stream(t: torch.Tensor) -> int:
    return torch.cuda.current_stream(t.device).cuda_stream if t.is_cuda else 0


def _p(t: Optional[torch.Tensor]) -> Optional[int]:
    return None if t is None else t.data_ptr()


def _ld(t: torch.Tensor) -> int:
    assert t.dim() == 2 and t.stride(1) == 1, "need a row-major 2-D view"
    return t.stride(0)


def _f32(*ts):
    for t in ts:
        assert t is None or (t.dtype == torch.float32 and t.is_contiguous()), "expected contiguous fp32"


def _i32(*ts):
    for t in ts:
        assert t.dtype == torch.int32 and t.is_contiguous(), "expected contiguous int32"


def _lens(lens, B):
    _i32(lens)
    assert lens.dim() == 1 and lens.shape[0] == B and lens.is_contiguous(), "lens must be a contiguous int32 [B]"


# ---------------------------------------------------------------- GEMMs
def gemm_nt(A, W, bias, C, epilogue=OD_EPI_NONE, accumulate=False, x3=False):
    code, W = mm_code(A.dtype, x3, W), _w(W)
    M, K = A.shape
    N = W.shape[0]
    assert W.shape[1] == K and tuple(C.shape) == (M, N)
    assert A.dtype == W.dtype == C.dtype
    _f32(bias)
    _lib.lib().od_gemm_nt(code, _p(A), _ld(A), _p(W), _ld(W), _p(bias), _p(C), _ld(C), M, N, K,
                          epilogue, int(accumulate), _stream(A))


def gemm_nt_qkrope(A, W, bias, C, wq, wk, table, L, H, hd, eps, x3=False, q_scale=1.0):
    """qkv projection with q/k RMSNorm + RoPE in the epilogue (forward-only): C[:, :2*H*hd] normed + rotated."""
    code, W = mm_code(A.dtype, x3, W), _w(W)
    M, K = A.shape
    N = W.shape[0]
    assert W.shape[1] == K and tuple(C.shape) == (M, N) and A.dtype == W.dtype == C.dtype
    _f32(bias, wq, wk, table)
    _lib.lib().od_gemm_nt_qkrope(code, _p(A), _ld(A), _p(W), _ld(W), _p(bias), _p(C), _ld(C), M, N, K,
                                 _p(wq), _p(wk), _p(table), L, H, hd, eps, q_scale, _stream(A))


def gemm_nt_qkrope_split(A, W, bias, C, qk_out, wq, wk, table, L, H, hd, eps, x3=False, q_scale=1.0):
    """qkv projection for training: C keeps the pre-norm values, qk_out[:, :2*H*hd] gets q/k normed + rotated."""
    code, W = mm_code(A.dtype, x3, W), _w(W)          # a weight pre-split for the fp32-as-3-x-bf16 product (pack_weights(x3=True)) arrives wrapped
    M, K = A.shape
    N = W.shape[0]
    assert W.shape[1] == K and tuple(C.shape) == (M, N) and tuple(qk_out.shape) == (M, 2 * H * hd)
    assert A.dtype == W.dtype == C.dtype
    # qk_out in torch.float16 = "attention in fp16": the roped q, k AND the v columns of C are then written as IEEE half
    # (C stays a bf16 tensor whose last N - 2*H*hd columns hold half bit patterns: view them with .view(torch.float16))
    assert qk_out.dtype == A.dtype or (qk_out.dtype == torch.float16 and A.dtype == torch.bfloat16)
    _f32(bias, wq, wk, table)
    qk_code = _lib.OD_F16 if qk_out.dtype == torch.float16 else (OD_F32 if A.dtype == torch.float32 else code)
    _lib.lib().od_gemm_nt_qkrope_split(code, _p(A), _ld(A), _p(W), _ld(W), _p(bias), _p(C), _ld(C), _p(qk_out),
                                       _ld(qk_out), qk_code, M, N, K, _p(wq), _p(wk), _p(table), L, H, hd, eps, q_scale, _stream(A))


def gemm_tn(G, A, dW, n_cols=None, k_cols=None, dbias=None, n_block=0, n_valid=0):
    """dW[N,K] += G[:, :N]^T A[:, :K] (and dbias[N] += column sums of G);  dW is any fp32 tensor
    viewed as [N, K] rows.  `n_block` / `n_valid`: G's columns come in blocks of n_block of which the first n_valid are live (the padded
    SwiGLU width); dW / dbias are then the UN-padded (N / n_block * n_valid) rows."""
    M = G.shape[0]
    N = n_cols if n_cols is not None else G.shape[1]
    K = k_cols if k_cols is not None else A.shape[1]
    rows = N if not n_block else (N // n_block) * n_valid
    assert not n_block or N % n_block == 0
    assert dW.dtype == torch.float32 and dW.is_contiguous() and dW.numel() == rows * K
    _f32(dbias)
    _lib.lib().od_gemm_tn_blocks(dt_code(G.dtype), _p(G), _ld(G), _p(A), _ld(A), _p(dW), K, _p(dbias), M, N, K, n_block, n_valid, _stream(G))


def colsum(G, out, n_cols=None):
    M = G.shape[0]
    N = n_cols if n_cols is not None else G.shape[1]
    _f32(out)
    _lib.lib().od_colsum(dt_code(G.dtype), _p(G), _ld(G), _p(out), M, N, _stream(G))


def pack_weight(src, dst, transpose=False, row_map=None):
    """dst (compute dtype, zero padded) from the fp32 master `src` viewed as [N, K].  A `SplitWeight` destination receives the
    pre-split (hi, lo) bf16 layout of OD_F32X3W (K padded to a multiple of 32, no transpose)."""
    N = src.shape[0]
    K = src.numel() // N
    _f32(src)
    code = OD_F32X3W if isinstance(dst, SplitWeight) else dt_code(_w(dst).dtype)
    dst = _w(dst)
    if transpose:
        Kp, Np = dst.shape
    else:
        Np, Kp = dst.shape
    assert dst.is_contiguous()
    _lib.lib().od_pack_weight(code, _p(src), N, K, _p(dst), Np, Kp, int(transpose), _p(row_map), _stream(src))


# ---------------------------------------------------------------- per-sample linears (fp32)
def linear_small(x, W, b, out, pre=None, act=OD_ACT_NONE):
    B, K = x.shape
    N = W.shape[0]
    _f32(x, W, b, out, pre)
    _lib.lib().od_linear_small(_p(x), _p(W), _p(b), _p(out), _p(pre), B, N, K, act, _stream(x))


def linear_small_bwd(x, W, pre, dout, dpre, dW, db, dx, accumulate_dx, act=OD_ACT_NONE):
    B, K = x.shape
    N = W.shape[0]
    _f32(x, W, pre, dout, dpre, dW, db, dx)
    _lib.lib().od_linear_small_bwd(_p(x), _p(W), _p(pre), _p(dout), _p(dpre), _p(dW), _p(db), _p(dx),
                                   int(accumulate_dx), B, N, K, act, _stream(x))


# ---------------------------------------------------------------- boundary / layout
def cl_to_frames(src, dst):
    B, C, L = src.shape
    _f32(src)
    _lib.lib().od_cl_to_frames(dt_code(dst.dtype), _p(src), _p(dst), _ld(dst), B, C, L, _stream(src))


def _feed_rows(base, cstride, lens, N):
    """The per-row descriptor both feed gathers read on the device: base / cstride int64 [N], lens int32 [N]."""
    assert lens.dtype == torch.int32 and lens.dim() == 1 and lens.shape[0] == N and lens.is_contiguous(), "lens must be a contiguous int32 [B]"
    for t in (base, cstride):
        assert t.dtype == torch.int64 and t.dim() == 1 and t.shape[0] == N and t.is_contiguous(), "base / cstride must be contiguous int64 [N]"


def feed_gather(store, base, cstride, lens, out):
    """out (N, C, Lpad) fp32 = per row n, lens[n] frames of C channels from the flat fp32 `store` at base[n] + c * cstride[n], zero beyond
    (base, cstride: device int64 [N]; lens: device int32 [N]).  Every element of out is written."""
    N, C, Lpad = out.shape
    _f32(store, out)
    _feed_rows(base, cstride, lens, N)
    assert store.device == out.device == base.device == cstride.device == lens.device, "feed_gather: every tensor on one device"
    _lib.lib().od_feed_gather(_p(store), store.numel(), _p(base), _p(cstride), _p(lens), _p(out), N, C, Lpad, _stream(out))


def feed_gather_quant(store, elem_size, base, cstride, lens, out, c0=0, channels=None, scale=None, offset=None, flip=None):
    """Channels c0 .. c0 + channels of out (N, Ctot, Lpad) fp32 = per row n, lens[n] frames of `channels` channels of unsigned integers of
    `elem_size` (1 or 2) bytes from the byte `store` (uint8, flat) at element base[n] + c * cstride[n], as double(q) / qmax * scale[n][c] +
    offset[n][c] rounded once to fp32 (scale / offset: device fp64 (N, channels), or both None), then 1 - v where bit c of flip[n] (device
    int32 [N], or None) is set; zero beyond lens[n].  Every element of those channels is written, no other."""
    N, Ctot, Lpad = out.shape
    C = Ctot - c0 if channels is None else channels
    _f32(out)
    _feed_rows(base, cstride, lens, N)
    assert store.dtype == torch.uint8 and store.dim() == 1 and store.is_contiguous(), "the store is a flat uint8 tensor (its bytes)"
    assert (scale is None) == (offset is None), "scale and offset come together"
    for t in (scale, offset):
        assert t is None or (t.dtype == torch.float64 and tuple(t.shape) == (N, C) and t.is_contiguous()), "scale / offset must be contiguous fp64 (N, channels)"
    if flip is not None:
        _lens(flip, N)
    assert all(t is None or t.device == out.device for t in (store, base, cstride, lens, scale, offset, flip)), "feed_gather_quant: every tensor on one device"
    _lib.lib().od_feed_gather_quant(_p(store), store.numel(), elem_size, _p(base), _p(cstride), _p(lens), _p(scale), _p(offset), _p(flip), _p(out),
                                    N, C, c0, Ctot, Lpad, _stream(out))


def replicate_tail(x, lens, plens):
    """x (N, C, Lpad) fp32, in place: frames lens[n] .. plens[n] of every channel of row n take the row's frame lens[n] - 1 (replicate
    padding; lens, plens: device int32 [N]).  Nothing else is written."""
    N, C, Lpad = x.shape
    _f32(x)
    _lens(lens, N)
    _lens(plens, N)
    assert x.device == lens.device == plens.device, "replicate_tail: every tensor on one device"
    _lib.lib().od_replicate_tail(_p(x), _p(lens), _p(plens), N, C, Lpad, _stream(x))


def proj_in(xt, W, bias, x):
    B, E, L = xt.shape
    D = x.shape[1]
    _f32(xt, W, bias)
    _lib.lib().od_proj_in(dt_code(x.dtype), _p(xt), _p(W), _p(bias), _p(x), _ld(x), B, E, L, D, _stream(xt))


def proj_in_bwd(xt, dx, dW, db):
    B, E, L = xt.shape
    D = dx.shape[1]
    _f32(xt, dW, db)
    _lib.lib().od_proj_in_bwd(dt_code(dx.dtype), _p(xt), _p(dx), _ld(dx), _p(dW), _p(db), B, E, L, D, _stream(xt))


def silu(x, y):
    assert x.is_contiguous() and y.is_contiguous()
    _lib.lib().od_silu(dt_code(x.dtype), _p(x), _p(y), x.numel(), _stream(x))


def silu_bwd(x, dy, dx):
    assert x.is_contiguous() and dy.is_contiguous() and dx.is_contiguous()
    _lib.lib().od_silu_bwd(dt_code(x.dtype), _p(x), _p(dy), _p(dx), x.numel(), _stream(x))


# ---------------------------------------------------------------- norm / modulation
def rmsnorm_film(x, ssg, cl, cl_bcast, h, inv_rms, B, L, eps=1e-6):
    C = x.shape[1]
    _f32(ssg, inv_rms)
    _lib.lib().od_rmsnorm_film(dt_code(x.dtype), _p(x), _ld(x), _p(ssg), _p(cl), _ld(cl) if cl is not None else 0,
                               int(cl_bcast), _p(h), _ld(h), _p(inv_rms), B, L, C, eps, _stream(x))


def rmsnorm_film_bwd(x, inv_rms, ssg, dh, dres, dssg, B, L):
    C = x.shape[1]
    _f32(ssg, inv_rms, dssg)
    _lib.lib().od_rmsnorm_film_bwd(dt_code(x.dtype), _p(x), _ld(x), _p(inv_rms), _p(ssg), _p(dh), _ld(dh), _p(dres),
                                   _ld(dres), _p(dssg), B, L, C, _stream(x))


def rmsnorm_gate_residual(x, h, ssg, xo, inv_rms, B, L, eps=1e-6):
    C = x.shape[1]
    _f32(ssg, inv_rms)
    _lib.lib().od_rmsnorm_gate_residual(dt_code(x.dtype), _p(x), _ld(x), _p(h), _ld(h), _p(ssg), _p(xo), _ld(xo),
                                        _p(inv_rms), B, L, C, eps, _stream(x))


def rmsnorm_gate_residual_film(x, h, ssg_a, xo, inv_a, ssg_b, cl, cl_bcast, h2, inv_b, B, L, eps=1e-6):
    """xo = x + rms(h) * gate_a;  h2 = rms(xo) * (1 + scale_b) + shift_b (+ cl)  — forward-only fused pair."""
    _f32(ssg_a, ssg_b, inv_a, inv_b)
    _lib.lib().od_rmsnorm_gate_residual_film(dt_code(x.dtype), _p(x), _ld(x), _p(h), _ld(h), _p(ssg_a), _p(xo), _ld(xo),
                                             _p(inv_a), _p(ssg_b), _p(cl), _ld(cl) if cl is not None else 0, int(cl_bcast),
                                             _p(h2), _ld(h2), _p(inv_b), B, L, x.shape[1], eps, _stream(x))


def rmsnorm_gate_residual_film_dwconv(x, h, ssg_a, xo, inv_a, ssg_b, h2, inv_b, conv_w, conv_b, y, B, L, ksize, eps=1e-6):
    """rmsnorm_gate_residual_film (no cl) and the depthwise conv of the SwiGLU branch in one pass: y = dwconv(h2) + b.  h2 may be None."""
    _f32(ssg_a, ssg_b, inv_a, inv_b, conv_w, conv_b)
    assert xo.data_ptr() != x.data_ptr() and xo.data_ptr() != h.data_ptr()
    _lib.lib().od_rmsnorm_gate_residual_film_dwconv(dt_code(x.dtype), _p(x), _ld(x), _p(h), _ld(h), _p(ssg_a), _p(xo), _ld(xo), _p(inv_a),
                                                    _p(ssg_b), _p(h2), _ld(h2) if h2 is not None else 0, _p(inv_b), _p(conv_w), _p(conv_b),
                                                    _p(y), _ld(y), B, L, x.shape[1], ksize, eps, _stream(x))


def rmsnorm_gate_residual_bwd(h, inv_rms, ssg, dy, dh, dssg, B, L):
    C = h.shape[1]
    _f32(ssg, inv_rms, dssg)
    _lib.lib().od_rmsnorm_gate_residual_bwd(dt_code(h.dtype), _p(h), _ld(h), _p(inv_rms), _p(ssg), _p(dy), _ld(dy),
                                            _p(dh), _ld(dh), _p(dssg), B, L, C, _stream(h))


# ---------------------------------------------------------------- attention
def rope_table(table, L, hd):
    _f32(table)
    _lib.lib().od_rope_table(_p(table), L, hd, _stream(table))


def qk_norm_rope(qkv, wq, wk, table, qk_out, B, L, H, hd, eps, q_scale=1.0):
    _f32(wq, wk, table)
    _lib.lib().od_qk_norm_rope(dt_code(qkv.dtype), _p(qkv), _ld(qkv), _p(wq), _p(wk), _p(table), _p(qk_out),
                               _ld(qk_out), B, L, H, hd, eps, q_scale, _stream(qkv))


def qk_norm_rope_bwd(qkv, wq, wk, table, dqk, dqkv, dwq, dwk, B, L, H, hd, eps, q_scale=1.0):
    _f32(wq, wk, table, dwq, dwk)
    _lib.lib().od_qk_norm_rope_bwd(dt_code(qkv.dtype), _p(qkv), _ld(qkv), _p(wq), _p(wk), _p(table), _p(dqk), _ld(dqk),
                                   _p(dqkv), _ld(dqkv), _p(dwq), _p(dwk), B, L, H, hd, eps, q_scale, _stream(qkv))


def flash_attn_fwd(q, k, v, o, lse, B, H, L, hd, scale, x3=False, q_prescaled=False):
    """q, k, v in torch.float16 (o stays bf16): the half-operand kernel ("attention in fp16")."""
    _f32(lse)
    assert q.dtype == k.dtype == v.dtype and (o.dtype == q.dtype or (q.dtype == torch.float16 and o.dtype == torch.bfloat16))
    _lib.lib().od_flash_attn_fwd(mm_code(q.dtype, x3), _p(q), _ld(q), _p(k), _ld(k), _p(v), _ld(v), _p(o), _ld(o), _p(lse),
                                 B, H, L, hd, scale, int(q_prescaled), _stream(q))


class AttnAux:
    """The side stream + events of the two-stream attention backward (od_attn_aux_create); owned by whoever plans the launches."""

    def __init__(self):
        import ctypes
        self.handle = ctypes.c_void_p()
        _lib.lib().od_attn_aux_create(ctypes.byref(self.handle))

    def close(self):
        if self.handle:
            _lib.lib().od_attn_aux_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def flash_attn_fwd_varlen(q, k, v, o, lse, lens, B, H, L, hd, scale, x3=False, q_prescaled=False):
    """flash_attn_fwd per sequence: lens (device int32 [B]) = valid rows of each sequence of the padded (B, L) layout.
    Rows >= lens[b] of o and lse come back as 0."""
    _f32(lse)
    _i32(lens)
    assert q.dtype == k.dtype == v.dtype and (o.dtype == q.dtype or (q.dtype == torch.float16 and o.dtype == torch.bfloat16))
    _lib.lib().od_flash_attn_fwd_varlen(mm_code(q.dtype, x3), _p(q), _ld(q), _p(k), _ld(k), _p(v), _ld(v), _p(o), _ld(o), _p(lse),
                                        _p(lens), B, H, L, hd, scale, int(q_prescaled), _stream(q))


def flash_attn_bwd(q, k, v, o, do, lse, delta, dq, dk, dv, B, H, L, hd, scale, q_prescaled=False, aux=None):
    _f32(lse, delta)
    _lib.lib().od_flash_attn_bwd_aux(dt_code(q.dtype), _p(q), _ld(q), _p(k), _ld(k), _p(v), _ld(v), _p(o), _ld(o), _p(do),
                                     _ld(do), _p(lse), _p(delta), _p(dq), _ld(dq), _p(dk), _ld(dk), _p(dv), _ld(dv),
                                     B, H, L, hd, scale, int(q_prescaled), aux.handle if aux is not None else None, _stream(q))


def flash_attn_bwd_varlen(q, k, v, o, do, lse, delta, dq, dk, dv, lens, B, H, L, hd, scale, q_prescaled=False, aux=None):
    """flash_attn_bwd per sequence (lens: device int32 [B]): rows >= lens[b] of q, k, v, do are never used and rows >= lens[b] of
    dq, dk, dv come back as exact zeros."""
    _f32(lse, delta)
    _i32(lens)
    _lib.lib().od_flash_attn_bwd_varlen(dt_code(q.dtype), _p(q), _ld(q), _p(k), _ld(k), _p(v), _ld(v), _p(o), _ld(o), _p(do),
                                        _ld(do), _p(lse), _p(delta), _p(dq), _ld(dq), _p(dk), _ld(dk), _p(dv), _ld(dv), _p(lens),
                                        B, H, L, hd, scale, int(q_prescaled), aux.handle if aux is not None else None, _stream(q))


class FusedAttnBwdWorkspace:
    """Caller-owned device memory of od_flash_attn_bwd_fused for one (B, H, L): control block + chain flags (zeroed once here; every call
    leaves them zero), the start values (-lse', -delta) and the running dQ tiles.  One instance serves every layer of a step (same stream)."""

    def __init__(self, B, H, L, device, dtype=torch.bfloat16):
        """`dtype` torch.float16: room for the staged half copy of dO as well ("attention in fp16")."""
        import ctypes
        total, zero = ctypes.c_long(), ctypes.c_long()
        _lib.lib().od_flash_attn_bwd_fused_ws_bytes(dt_code(dtype), B, H, L, ctypes.byref(total), ctypes.byref(zero))
        self.shape = (B, H, L)
        self.dtype = dtype
        self.bytes = total.value
        assert zero.value <= self.bytes
        self.zero_bytes = zero.value
        self.buf = torch.empty(self.bytes, dtype=torch.uint8, device=device)
        self.reset()

    def reset(self):
        """Zero the control block and the running tiles (a zero tile carries write number 0): once at creation, and again after a status-3 launch."""
        self.buf[:self.zero_bytes].zero_()

    def err_ptr(self) -> int:
        """Device address of the sticky error word: ops.sqnorm / ops.adamw_ema fold it into the step without a host round trip."""
        return self.buf.data_ptr() + int(_lib.lib().cdll.od_flash_attn_bwd_fused_err_offset())

    def err_view(self) -> torch.Tensor:
        """The sticky error word as an int32[1] tensor (a view of the workspace): what a data-parallel step reduces over the ranks."""
        off = int(_lib.lib().cdll.od_flash_attn_bwd_fused_err_offset())
        return self.buf[off:off + 4].view(torch.int32)

    def status(self) -> int:
        """The sticky error word (0 = every launch processed all of its jobs; 1 / 2 / 3: see the header).  Waits for the current stream."""
        import ctypes
        err = ctypes.c_int(-1)
        _lib.lib().od_flash_attn_bwd_fused_status(_p(self.buf), ctypes.byref(err), _stream(self.buf))
        return err.value


def flash_attn_bwd_fused(q, k, v, o, do, lse, dq, dk, dv, B, H, L, hd, scale, ws: FusedAttnBwdWorkspace, q_prescaled=False):
    """The 5-pass fused attention backward (bf16, head_dim 64): dq, dk, dv from one kernel, dQ summed over key blocks by the L2 chain.
    q, k, v in torch.float16: the half-operand form (o, do, dq, dk, dv stay bf16; the workspace must have been made for float16)."""
    _f32(lse)
    assert ws.shape == (B, H, L), (ws.shape, (B, H, L))
    assert q.dtype == k.dtype == v.dtype and o.dtype == do.dtype == dq.dtype == dk.dtype == dv.dtype == torch.bfloat16
    assert q.dtype == torch.bfloat16 or (q.dtype == torch.float16 and ws.dtype == torch.float16)
    _lib.lib().od_flash_attn_bwd_fused(dt_code(q.dtype), _p(q), _ld(q), _p(k), _ld(k), _p(v), _ld(v), _p(o), _ld(o), _p(do), _ld(do),
                                       _p(lse), _p(dq), _ld(dq), _p(dk), _ld(dk), _p(dv), _ld(dv), B, H, L, hd, scale, int(q_prescaled),
                                       _p(ws.buf), ws.bytes, _stream(q))


# ---------------------------------------------------------------- feed-forward
def dwconv(x, w, bias, y, B, L, ksize, lens=None):
    """`lens` (device int32 [B]): per sequence of valid length lens[b]; frames >= lens[b] of y come back as 0."""
    C = x.shape[1]
    _f32(w, bias)
    if lens is None:
        return _lib.lib().od_dwconv(dt_code(x.dtype), _p(x), _ld(x), _p(w), _p(bias), _p(y), _ld(y), B, L, C, ksize, _stream(x))
    _i32(lens)
    _lib.lib().od_dwconv_varlen(dt_code(x.dtype), _p(x), _ld(x), _p(w), _p(bias), _p(y), _ld(y), _p(lens), B, L, C, ksize, _stream(x))


def dwconv_varlen(x, w, bias, y, lens, B, L, ksize):
    dwconv(x, w, bias, y, B, L, ksize, lens)


def dwconv_bwd(x, w, dy, dx, dw, db, B, L, ksize):
    C = x.shape[1]
    _f32(w, dw, db)
    _lib.lib().od_dwconv_bwd(dt_code(x.dtype), _p(x), _ld(x), _p(w), _p(dy), _ld(dy), _p(dx), _ld(dx), _p(dw), _p(db),
                             B, L, C, ksize, _stream(x))


def dwconv_bwd_varlen(x, w, dy, dx, dw, db, lens, B, L, ksize):
    """dwconv_bwd per sequence of valid length lens[b] (device int32 [B]); frames >= lens[b] of dx come back as 0."""
    C = x.shape[1]
    _f32(w, dw, db)
    _i32(lens)
    _lib.lib().od_dwconv_bwd_varlen(dt_code(x.dtype), _p(x), _ld(x), _p(w), _p(dy), _ld(dy), _p(dx), _ld(dx), _p(dw), _p(db),
                                    _p(lens), B, L, C, ksize, _stream(x))


def scale_channels(x, scale, B, L):
    """x[(b, l), c] *= scale[b, c] in place (Dropout1d's channel mask; also its backward)."""
    _f32(scale)
    assert scale.shape == (B, x.shape[1]) and scale.is_contiguous()
    _lib.lib().od_scale_channels(dt_code(x.dtype), _p(x), _ld(x), _p(scale), B, L, x.shape[1], _stream(x))


def swiglu_rmsnorm(vg, hh, inv_rms, Hf, Hp, eps=1e-6):
    _f32(inv_rms)
    _lib.lib().od_swiglu_rmsnorm(dt_code(vg.dtype), _p(vg), _ld(vg), _p(hh), _ld(hh), _p(inv_rms), vg.shape[0], Hf, Hp,
                                 eps, _stream(vg))


def swiglu_rmsnorm_bwd(vg, inv_rms, dhh, dvg, Hf, Hp):
    _f32(inv_rms)
    _lib.lib().od_swiglu_rmsnorm_bwd(dt_code(vg.dtype), _p(vg), _ld(vg), _p(inv_rms), _p(dhh), _ld(dhh), _p(dvg),
                                     _ld(dvg), vg.shape[0], Hf, Hp, _stream(vg))


# ---------------------------------------------------------------- heads
def final_norm_proj_out(x, W, bias, v, inv_rms, B, L, eps=1e-6):
    C = x.shape[1]
    E = W.shape[0]
    _f32(W, bias, v, inv_rms)
    _lib.lib().od_final_norm_proj_out(dt_code(x.dtype), _p(x), _ld(x), _p(W), _p(bias), _p(v), _p(inv_rms), B, L, C, E,
                                      eps, _stream(x))


def final_norm_proj_out_bwd(x, inv_rms, W, dv, dx, dW, db, B, L):
    C = x.shape[1]
    E = W.shape[0]
    _f32(W, dv, inv_rms, dW, db)
    _lib.lib().od_final_norm_proj_out_bwd(dt_code(x.dtype), _p(x), _ld(x), _p(inv_rms), _p(W), _p(dv), _p(dx), _ld(dx),
                                          _p(dW), _p(db), B, L, C, E, _stream(x))


def uhead_fwd(xt, w, fsum, U):
    """w: the eight u_head tensors (w0,b0,w1,b1,w3,b3,w4,b4)."""
    B, E, L = xt.shape
    _f32(xt, fsum, *w)
    _lib.lib().od_uhead_fwd(_p(xt), *[_p(t) for t in w], _p(fsum), B, E, L, U, _stream(xt))


def uhead_fwd_varlen(xt, w, fsum, lens, U):
    B, E, L = xt.shape
    _f32(xt, fsum, *w)
    _i32(lens)
    _lib.lib().od_uhead_fwd_varlen(_p(xt), *[_p(t) for t in w], _p(fsum), _p(lens), B, E, L, U, _stream(xt))


def uhead_bwd(xt, w, dfm, g, U):
    B, E, L = xt.shape
    _f32(xt, dfm, *w, *g)
    _lib.lib().od_uhead_bwd(_p(xt), *[_p(t) for t in w], _p(dfm), *[_p(t) for t in g], B, E, L, U, _stream(xt))


def uhead_bwd_varlen(xt, w, dfm, g, lens, U):
    B, E, L = xt.shape
    _f32(xt, dfm, *w, *g)
    _i32(lens)
    _lib.lib().od_uhead_bwd_varlen(_p(xt), *[_p(t) for t in w], _p(dfm), *[_p(t) for t in g], _p(lens), B, E, L, U, _stream(xt))


def uhead_tail(fsum, mod, w_out, b_out, u, L, u_scale):
    B, U = fsum.shape
    _f32(fsum, mod, w_out, b_out, u)
    _lib.lib().od_uhead_tail(_p(fsum), _p(mod), _p(w_out), _p(b_out), _p(u), B, U, L, u_scale, _stream(fsum))


def uhead_tail_varlen(fsum, mod, w_out, b_out, u, lens, L, u_scale):
    B, U = fsum.shape
    _f32(fsum, mod, w_out, b_out, u)
    _i32(lens)
    _lib.lib().od_uhead_tail_varlen(_p(fsum), _p(mod), _p(w_out), _p(b_out), _p(u), _p(lens), B, U, L, u_scale, _stream(fsum))


def uhead_tail_bwd(fsum, mod, w_out, b_out, du, dfm, dmod, dw_out, db_out, L, u_scale):
    B, U = fsum.shape
    _f32(fsum, mod, w_out, b_out, du, dfm, dmod, dw_out, db_out)
    _lib.lib().od_uhead_tail_bwd(_p(fsum), _p(mod), _p(w_out), _p(b_out), _p(du), _p(dfm), _p(dmod), _p(dw_out),
                                 _p(db_out), B, U, L, u_scale, _stream(fsum))


def uhead_tail_bwd_varlen(fsum, mod, w_out, b_out, du, dfm, dmod, dw_out, db_out, lens, L, u_scale):
    B, U = fsum.shape
    _f32(fsum, mod, w_out, b_out, du, dfm, dmod, dw_out, db_out)
    _i32(lens)
    _lib.lib().od_uhead_tail_bwd_varlen(_p(fsum), _p(mod), _p(w_out), _p(b_out), _p(du), _p(dfm), _p(dmod), _p(dw_out),
                                        _p(db_out), _p(lens), B, U, L, u_scale, _stream(fsum))


# ---------------------------------------------------------------- loss / sampler
def make_xt(x0, x1, t, xt, dsq):
    B, E, L = x0.shape
    _f32(x0, x1, t, xt, dsq)
    _lib.lib().od_make_xt(_p(x0), _p(x1), _p(t), _p(xt), _p(dsq), B, E, L, _stream(x0))


def make_xt_varlen(x0, x1, t, xt, dsq, lens):
    """make_xt per sequence (lens: device int32 [B]): dsq[b] over frames < lens[b]; xt = 0 at frames >= lens[b], where x0 / x1 are not read."""
    B, E, L = x0.shape
    _f32(x0, x1, t, xt, dsq)
    _i32(lens)
    _lib.lib().od_make_xt_varlen(_p(x0), _p(x1), _p(t), _p(xt), _p(dsq), _p(lens), B, E, L, _stream(x0))


def loss_grad(xt, x1, u, v, dsq, dv, sums, c0, osl_w, del_w):
    B, E, L = xt.shape
    _f32(xt, x1, u, v, dsq, dv, sums)
    _lib.lib().od_loss_grad(_p(xt), _p(x1), _p(u), _p(v), _p(dsq), _p(dv), _p(sums), B, E, L, c0, osl_w, del_w, _stream(xt))


def loss_grad_varlen(xt, x1, u, v, dsq, dv, sums, lens, c0, osl_w, del_w):
    """loss_grad per sequence: sums over frames < lens[b], normalised by lens[b]; dv = 0 at frames >= lens[b]."""
    B, E, L = xt.shape
    _f32(xt, x1, u, v, dsq, dv, sums)
    _i32(lens)
    _lib.lib().od_loss_grad_varlen(_p(xt), _p(x1), _p(u), _p(v), _p(dsq), _p(dv), _p(sums), _p(lens), B, E, L, c0, osl_w, del_w,
                                   _stream(xt))


def loss_finalize(sums, dsq, u, out, du, c0, osl_w, del_w):
    B = u.shape[0]
    _f32(sums, dsq, u, out, du)
    _lib.lib().od_loss_finalize(_p(sums), _p(dsq), _p(u), _p(out), _p(du), B, c0, osl_w, del_w, _stream(u))


def loss_finalize_groups(sums, dsq, u, offs, out, c0, osl_w, del_w):
    """out (G, 4): per map g, loss_finalize's (loss, osl, del, u_mape) over rows [offs[g], offs[g+1]) of sums / dsq / u alone, bit for bit.
    offs: G + 1 host ints (a sequence, or an int32 tensor on the host) that cover rows of u only; an empty map is refused."""
    _f32(sums, dsq, u, out)
    offs = torch.as_tensor(offs, dtype=torch.int32).contiguous()
    assert offs.device.type == "cpu" and offs.dim() == 1 and offs.numel() >= 1, "offs: G + 1 ints on the host"
    G = offs.numel() - 1
    assert out.numel() >= 4 * G and int(offs[-1]) <= u.shape[0] and sums.numel() >= 3 * u.shape[0] and dsq.numel() >= u.shape[0]
    _lib.lib().od_loss_finalize_groups(_p(sums), _p(dsq), _p(u), _p(offs), _p(out), G, c0, osl_w, del_w, _stream(u))


def sampler_step(x, u, v, eta):
    B, E, L = x.shape
    _f32(x, u, v, eta)
    _lib.lib().od_sampler_step(_p(x), _p(u), _p(v), _p(eta), B, E, L, _stream(x))


def sampler_eta(u, eta, c0, num_steps):
    _f32(u, eta)
    _lib.lib().od_sampler_eta(_p(u), _p(eta), u.shape[0], c0, num_steps, _stream(u))


def sampler_eta_groups(u, offs, eta, c0, num_steps):
    """eta (G, 2): per song g, sampler_eta over rows [offs[g], offs[g+1]) of u (offs: device int32 [G+1])."""
    _f32(u, eta)
    _i32(offs)
    G = offs.shape[0] - 1
    assert eta.numel() >= 2 * G
    _lib.lib().od_sampler_eta_groups(_p(u), _p(offs), _p(eta), G, c0, num_steps, _stream(u))


def sampler_step_varlen(x, u, v, eta, lens, offs):
    B, E, L = x.shape
    _f32(x, u, v, eta)
    _i32(lens, offs)
    _lib.lib().od_sampler_step_varlen(_p(x), _p(u), _p(v), _p(eta), _p(lens), _p(offs), offs.shape[0] - 1, B, E, L, _stream(x))


# ---------------------------------------------------------------- optimizer
def sqnorm(g, out, status_ptr: int = 0):
    """out[0] += sum g^2; `status_ptr` (a device address, 0 = none): non-zero error word -> out[0] = NaN, on the device."""
    _f32(g, out)
    _lib.lib().od_sqnorm(_p(g), g.numel(), _p(out), status_ptr or None, _stream(g))


def adamw_ema(p, g, m, v, ema, lr, beta1, beta2, eps, weight_decay, step, ema_decay, ema_mode, gnorm_sq, max_norm, status_ptr: int = 0):
    _f32(p, g, m, v, ema, gnorm_sq)
    _lib.lib().od_adamw_ema(_p(p), _p(g), _p(m), _p(v), _p(ema), p.numel(), lr, beta1, beta2, eps, weight_decay, step,
                            ema_decay, ema_mode, _p(gnorm_sq), max_norm, status_ptr or None, _stream(p))


def ema_update(ema, p, decay, mode):
    _f32(ema, p)
    _lib.lib().od_ema_update(_p(ema), _p(p), p.numel(), decay, mode, _stream(p))


# ---------------------------------------------------------------- style model
def style_conditioning(labels, rff_w, rff_b, cond_w, cond_b, null_labels, c):
    B, NL = labels.shape
    F, H = cond_w.shape[1], cond_w.shape[2]
    _f32(labels, rff_w, rff_b, cond_w, cond_b, null_labels, c)
    _lib.lib().od_style_conditioning(_p(labels), _p(rff_w), _p(rff_b), _p(cond_w), _p(cond_b), _p(null_labels), _p(c),
                                     B, NL, F, H, _stream(labels))


def rmsnorm_rows(x, gamma, y, eps):
    M, C = x.shape
    _f32(x, gamma, y)
    _lib.lib().od_rmsnorm_rows(_p(x), _p(gamma), _p(y), M, C, eps, _stream(x))


def style_conditioning_bwd(labels, rff_w, rff_b, dc, dcond_w, dcond_b, dnull_labels):
    """dcond_w / dcond_b / dnull_labels += the conditioning's parameter gradients under dc (B, H)."""
    B, NL = labels.shape
    F, H = dcond_w.shape[1], dcond_w.shape[2]
    _f32(labels, rff_w, rff_b, dc, dcond_w, dcond_b, dnull_labels)
    assert tuple(dc.shape) == (B, H) and rff_w.numel() == F and rff_b.numel() == F
    assert tuple(dcond_w.shape) == (NL, F, H) and tuple(dcond_b.shape) == (NL, H) and tuple(dnull_labels.shape) == (NL, H)
    _lib.lib().od_style_conditioning_bwd(_p(labels), _p(rff_w), _p(rff_b), _p(dc), _p(dcond_w), _p(dcond_b), _p(dnull_labels),
                                         B, NL, F, H, _stream(labels))


def rmsnorm_rows_bwd(x, gamma, dy, dx, dgamma, eps, accumulate_dx=False):
    """dx (+)= backward of rmsnorm_rows under dy; dgamma += (None when gamma is None)."""
    M, C = x.shape
    _f32(x, gamma, dy, dx, dgamma)
    assert dy.shape == x.shape == dx.shape and (gamma is None or gamma.numel() == C) and (dgamma is None or dgamma.numel() == C)
    _lib.lib().od_rmsnorm_rows_bwd(_p(x), _p(gamma), _p(dy), _p(dx), _p(dgamma), M, C, eps, int(accumulate_dx), _stream(x))


def cast_rows(src, dst):
    """dst = src converted between fp32 and bf16 (same shape, both contiguous)."""
    assert src.is_contiguous() and dst.is_contiguous() and src.numel() == dst.numel()
    _lib.lib().od_cast_rows(dt_code(src.dtype), _p(src), dt_code(dst.dtype), _p(dst), src.numel(), _stream(src))


# ---------------------------------------------------------------- latent model, forward.  `lens` (device int32 [B], the valid frames
# of each sequence at the level the call reads) selects the varlen entry point: frames past them come back as exact zeros
def spec_features_conv(audio, w1, b1, g1, w2, b2, g2, out, eps=1e-6, lens=None):
    B, F, L = audio.shape
    _f32(audio, w1, b1, g1, w2, b2, g2)
    if lens is None:
        return _lib.lib().od_spec_features_conv(dt_code(out.dtype), _p(audio), _p(w1), _p(b1), _p(g1), _p(w2), _p(b2), _p(g2),
                                                _p(out), _ld(out), B, F, L, eps, _stream(audio))
    _lens(lens, B)
    _lib.lib().od_spec_features_conv_varlen(dt_code(out.dtype), _p(audio), _p(w1), _p(b1), _p(g1), _p(w2), _p(b2), _p(g2),
                                            _p(out), _ld(out), _p(lens), B, F, L, eps, _stream(audio))


def rmsnorm_affine_film(x, gamma, ssg, y, B, L, act=OD_ACT_NONE, eps=1e-6, lens=None):
    _f32(gamma, ssg)
    if lens is None:
        return _lib.lib().od_rmsnorm_affine_film(dt_code(x.dtype), _p(x), _ld(x), _p(gamma), _p(ssg), _p(y), _ld(y), B, L, x.shape[1],
                                                 eps, act, _stream(x))
    _lens(lens, B)
    _lib.lib().od_rmsnorm_affine_film_varlen(dt_code(x.dtype), _p(x), _ld(x), _p(gamma), _p(ssg), _p(y), _ld(y), _p(lens), B, L,
                                             x.shape[1], eps, act, _stream(x))


def rmsnorm_affine_gate_residual(x, h, gamma, ssg, xo, B, L, eps=1e-6):
    _f32(gamma, ssg)
    _lib.lib().od_rmsnorm_affine_gate_residual(dt_code(x.dtype), _p(x), _ld(x), _p(h), _ld(h), _p(gamma), _p(ssg), _p(xo),
                                               _ld(xo), B, L, x.shape[1], eps, _stream(x))


def unet_mixer(x, p, p_bcast, gx, gamma, xo, B, L, eps=1e-6, prow=None):
    """`prow` (device int32 [B]): decoder row b reads frame l of skip row prow[b], and p_bcast is not looked at."""
    _f32(gamma)
    if prow is None:
        return _lib.lib().od_unet_mixer(dt_code(x.dtype), _p(x), _ld(x), _p(p), _ld(p), int(p_bcast), _p(gx), _ld(gx), _p(gamma),
                                        _p(xo), _ld(xo), B, L, x.shape[1], eps, _stream(x))
    _lens(prow, B)
    _lib.lib().od_unet_mixer_varlen(dt_code(x.dtype), _p(x), _ld(x), _p(p), _ld(p), _p(prow), _p(gx), _ld(gx), _p(gamma),
                                    _p(xo), _ld(xo), B, L, x.shape[1], eps, _stream(x))


def unet_down(x, w, bias, y, B, Lo, stride, lens=None):
    """lens: valid frames at the INPUT level (Lo * stride)."""
    _f32(w, bias)
    if lens is None:
        return _lib.lib().od_unet_down(dt_code(x.dtype), _p(x), _ld(x), _p(w), _p(bias), _p(y), _ld(y), B, Lo, x.shape[1], stride,
                                       _stream(x))
    _lens(lens, B)
    _lib.lib().od_unet_down_varlen(dt_code(x.dtype), _p(x), _ld(x), _p(w), _p(bias), _p(y), _ld(y), _p(lens), B, Lo, x.shape[1],
                                   stride, _stream(x))


def unet_up(x, w, bias, y, B, Li, stride, lens=None):
    """lens: valid frames at the INPUT level (Li)."""
    _f32(w, bias)
    if lens is None:
        return _lib.lib().od_unet_up(dt_code(x.dtype), _p(x), _ld(x), _p(w), _p(bias), _p(y), _ld(y), B, Li, x.shape[1], stride,
                                     _stream(x))
    _lens(lens, B)
    _lib.lib().od_unet_up_varlen(dt_code(x.dtype), _p(x), _ld(x), _p(w), _p(bias), _p(y), _ld(y), _p(lens), B, Li, x.shape[1],
                                 stride, _stream(x))


def chart_head(x, W, bias, out, B, L, n_sigmoid, rms=False, eps=1e-6, lens=None):
    _f32(W, bias, out)
    N = W.shape[0]
    if lens is None:
        return _lib.lib().od_chart_head(dt_code(x.dtype), _p(x), _ld(x), _p(W), _p(bias), _p(out), B, L, x.shape[1], N, n_sigmoid,
                                        int(rms), eps, _stream(x))
    _lens(lens, B)
    _lib.lib().od_chart_head_varlen(dt_code(x.dtype), _p(x), _ld(x), _p(W), _p(bias), _p(out), _p(lens), B, L, x.shape[1], N,
                                    n_sigmoid, int(rms), eps, _stream(x))


def attn_pool(scores, values, out, B, L, heads, hd, lens=None):
    _f32(out)
    if lens is None:
        return _lib.lib().od_attn_pool(dt_code(scores.dtype), _p(scores), _ld(scores), _p(values), _ld(values), _p(out), B, L, heads,
                                       hd, _stream(scores))
    _lens(lens, B)
    _lib.lib().od_attn_pool_varlen(dt_code(scores.dtype), _p(scores), _ld(scores), _p(values), _ld(values), _p(out), _p(lens), B, L,
                                   heads, hd, _stream(scores))


# ---------------------------------------------------------------- latent model, backward kernels.  Sums over frames (dgamma, dssg, dw,
# db, dW) are fp32 and ADDED to their destination, in a fixed order: `ws` is fp32 scratch for the per-block partial rows, at least
# latent_bwd_ws_floats(...) long.
def latent_bwd_ws_floats(kind, B, L, C, n=0):
    """Scratch floats of one backward call: kind 'film' / 'gate' / 'mixer' (n = 1: the skip is broadcast) with L the frames per batch
    row; 'down' / 'up' with L the frames of dy per batch row and n the stride; 'head' with n the output channels; 'spec' (C unused)."""
    if kind == "spec":
        return B * -(-L // 32) * 4880
    f = _lib.lib().cdll.od_latent_bwd_block_frames(C)
    assert f > 0, "C must be a power of two in 8..512"
    per_row, flat = -(-L // f), -(-(B * L) // f)
    if kind == "film":
        return B * per_row * 3 * C
    if kind == "gate":
        return B * per_row * 2 * C
    if kind == "mixer":
        return (per_row if n else B * per_row) * C
    if kind in ("down", "up"):
        return flat * (2 * (n // 2) + 2) * C
    if kind == "head":
        return flat * n * (C + 1)
    raise ValueError(kind)


def rmsnorm_affine_film_bwd(x, gamma, ssg, dy, dx, dgamma, dssg, ws, B, L, act=OD_ACT_NONE, accumulate_dx=False, eps=1e-6):
    """dx (+)= ; dgamma += ; dssg[:, :2C] += (ssg None: dssg unused) — backward of rmsnorm_affine_film under dy."""
    _f32(gamma, ssg, dgamma, dssg, ws)
    assert x.dtype == dy.dtype == dx.dtype
    _lib.lib().od_rmsnorm_affine_film_bwd(dt_code(x.dtype), _p(x), _ld(x), _p(gamma), _p(ssg), _p(dy), _ld(dy), _p(dx), _ld(dx),
                                          int(accumulate_dx), _p(dgamma), _p(dssg), _p(ws), ws.numel(), B, L, x.shape[1], eps, act,
                                          _stream(x))


def rmsnorm_affine_gate_residual_bwd(h, gamma, ssg, dxo, dh, dgamma, dssg, ws, B, L, eps=1e-6):
    """dh ; dgamma += ; dssg[:, 2C:] += (ssg None: dssg unused) — backward of rmsnorm_affine_gate_residual under dxo (dx is dxo)."""
    _f32(gamma, ssg, dgamma, dssg, ws)
    assert h.dtype == dxo.dtype == dh.dtype
    _lib.lib().od_rmsnorm_affine_gate_residual_bwd(dt_code(h.dtype), _p(h), _ld(h), _p(gamma), _p(ssg), _p(dxo), _ld(dxo), _p(dh),
                                                   _ld(dh), _p(dgamma), _p(dssg), _p(ws), ws.numel(), B, L, h.shape[1], eps, _stream(h))


def unet_mixer_bwd(p, p_bcast, gx, gamma, dxo, dp, dgx, dgamma, ws, B, L, eps=1e-6):
    """dgx ; dgamma += ; dp: [B*L, C] of the activation type, or fp32 [L, C] summed over the batch when p_bcast (dx is dxo)."""
    _f32(gamma, dgamma, ws)
    assert p.dtype == gx.dtype == dxo.dtype == dgx.dtype and dp.dtype == (torch.float32 if p_bcast else p.dtype)
    _lib.lib().od_unet_mixer_bwd(dt_code(p.dtype), _p(p), _ld(p), int(p_bcast), _p(gx), _ld(gx), _p(gamma), _p(dxo), _ld(dxo), _p(dp),
                                 _ld(dp), _p(dgx), _ld(dgx), _p(dgamma), _p(ws), ws.numel(), B, L, p.shape[1], eps, _stream(p))


def unet_down_bwd(x, w, dy, dx, dw, db, ws, B, Lo, stride):
    _f32(w, dw, db, ws)
    assert x.dtype == dy.dtype == dx.dtype
    _lib.lib().od_unet_down_bwd(dt_code(x.dtype), _p(x), _ld(x), _p(w), _p(dy), _ld(dy), _p(dx), _ld(dx), _p(dw), _p(db), _p(ws),
                                ws.numel(), B, Lo, x.shape[1], stride, _stream(x))


def unet_up_bwd(x, w, dy, dx, dw, db, ws, B, Li, stride):
    _f32(w, dw, db, ws)
    assert x.dtype == dy.dtype == dx.dtype
    _lib.lib().od_unet_up_bwd(dt_code(x.dtype), _p(x), _ld(x), _p(w), _p(dy), _ld(dy), _p(dx), _ld(dx), _p(dw), _p(db), _p(ws),
                              ws.numel(), B, Li, x.shape[1], stride, _stream(x))


def chart_head_bwd(x, W, bias, dout, dx, dW, db, ws, B, L, rms=False, eps=1e-6):
    """dx ; dW += ; db += — backward of chart_head(n_sigmoid = 0) under dout (B, N, L) fp32."""
    _f32(W, bias, dout, dW, db, ws)
    N = W.shape[0]
    assert tuple(dout.shape) == (B, N, L) and x.dtype == dx.dtype
    _lib.lib().od_chart_head_bwd(dt_code(x.dtype), _p(x), _ld(x), _p(W), _p(bias), _p(dout), _p(dx), _ld(dx), _p(dW), _p(db), _p(ws),
                                 ws.numel(), B, L, x.shape[1], N, int(rms), eps, _stream(x))


def attn_pool_bwd(scores, values, dout, dscores, dvalues, B, L, heads, hd):
    _f32(dout)
    assert scores.dtype == values.dtype == dscores.dtype == dvalues.dtype
    _lib.lib().od_attn_pool_bwd(dt_code(scores.dtype), _p(scores), _ld(scores), _p(values), _ld(values), _p(dout), _p(dscores),
                                _ld(dscores), _p(dvalues), _ld(dvalues), B, L, heads, hd, _stream(scores))


def spec_features_conv_bwd(audio, w1, b1, g1, w2, b2, g2, dout, dw1, db1, dg1, dw2, db2, dg2, ws, eps=1e-6):
    """dw1, db1, dg1, dw2, db2, dg2 += under dout [B*L, 96]; ws: at least latent_bwd_ws_floats('spec', B, L, 0) floats."""
    B, F, L = audio.shape
    _f32(audio, w1, b1, g1, w2, b2, g2, dw1, db1, dg1, dw2, db2, dg2, ws)
    _lib.lib().od_spec_features_conv_bwd(dt_code(dout.dtype), _p(audio), _p(w1), _p(b1), _p(g1), _p(w2), _p(b2), _p(g2), _p(dout),
                                         _ld(dout), _p(dw1), _p(db1), _p(dg1), _p(dw2), _p(db2), _p(dg2), _p(ws), ws.numel(), B, F, L,
                                         eps, _stream(audio))


def add_rows(x, y):
    """y += x (same dtype and shape, both contiguous)."""
    assert x.dtype == y.dtype and x.shape == y.shape and x.is_contiguous() and y.is_contiguous()
    _lib.lib().od_add_rows(dt_code(x.dtype), _p(x), _p(y), x.numel(), _stream(x))


def proj_in_bwd_input(dx, W, dxt):
    """dxt (B, E, L) fp32 = W^T dx: the gradient of proj_in's input."""
    B, E, L = dxt.shape
    _f32(W, dxt)
    _lib.lib().od_proj_in_bwd_input(dt_code(dx.dtype), _p(dx), _ld(dx), _p(W), _p(dxt), B, E, L, dx.shape[1], _stream(dx))


# ---------------------------------------------------------------- latent model, varlen names: the forward wrappers above with `lens`
def spec_features_conv_varlen(audio, w1, b1, g1, w2, b2, g2, out, lens, eps=1e-6):
    spec_features_conv(audio, w1, b1, g1, w2, b2, g2, out, eps, lens)


def rmsnorm_affine_film_varlen(x, gamma, ssg, y, lens, B, L, act=OD_ACT_NONE, eps=1e-6):
    rmsnorm_affine_film(x, gamma, ssg, y, B, L, act, eps, lens)


def unet_mixer_varlen(x, p, prow, gx, gamma, xo, B, L, eps=1e-6):
    unet_mixer(x, p, False, gx, gamma, xo, B, L, eps, prow)


def unet_down_varlen(x, w, bias, y, lens, B, Lo, stride):
    unet_down(x, w, bias, y, B, Lo, stride, lens)


def unet_up_varlen(x, w, bias, y, lens, B, Li, stride):
    unet_up(x, w, bias, y, B, Li, stride, lens)


def chart_head_varlen(x, W, bias, out, lens, B, L, n_sigmoid, rms=False, eps=1e-6):
    chart_head(x, W, bias, out, B, L, n_sigmoid, rms, eps, lens)


def attn_pool_varlen(scores, values, out, lens, B, L, heads, hd):
    attn_pool(scores, values, out, B, L, heads, hd, lens)


# ---------------------------------------------------------------- latent model, training-step kernels (fp32; deterministic sums)
def _u8(*ts):
    for t in ts:
        assert t.dtype == torch.uint8 and t.is_contiguous(), "expected contiguous uint8"


def mmd_imq(z, prior, out, dz, ws):
    """out[0] = MMD^2(z, prior) with the seven IMQ kernels, out[1:4] = its zz / pp / zp terms; dz = its gradient with respect to z."""
    N, D = z.shape
    _f32(z, prior, out, dz, ws)
    assert prior.shape == z.shape == dz.shape and out.numel() >= 4
    _lib.lib().od_mmd_imq(_p(z), _p(prior), _p(out), _p(dz), _p(ws), ws.numel(), N, D, _stream(z))


def scale_by(x, g, y):
    """y = x * g[0] (g: a device scalar)."""
    _f32(x, g, y)
    assert x.shape == y.shape
    _lib.lib().od_scale_by(_p(x), _p(g), _p(y), x.numel(), _stream(x))


def latent_perturb(z, s, eps_z, eps_s, u_s, repl, u_span, u_start, z_out, s_out, masked, start_span, s_noise, z_noise, s_mask_frac,
                   z_mask_frac, training):
    """z (B2, E, l) fp32 with any strides; everything else contiguous.  The draws may be None in eval mode (only the swap happens)."""
    B2, E, l = z.shape
    S = s.shape[1]
    assert z.dtype == torch.float32
    _f32(s, eps_z, eps_s, u_s, repl, u_span, u_start, z_out, s_out)
    _u8(masked)
    _i32(start_span)
    assert tuple(z_out.shape) == (B2, E, l) and tuple(s_out.shape) == (B2, S) and masked.numel() == B2 and start_span.numel() == 2 * B2
    _lib.lib().od_latent_perturb(_p(z), z.stride(0), z.stride(1), z.stride(2), _p(s), _p(eps_z), _p(eps_s), _p(u_s), _p(repl), _p(u_span),
                                 _p(u_start), _p(z_out), _p(s_out), _p(masked), _p(start_span), B2, E, l, S, s_noise, z_noise,
                                 s_mask_frac, z_mask_frac, int(training), _stream(s))


def latent_perturb_bwd(dz_out, ds_out, masked, start_span, dz, ds):
    B2, E, l = dz_out.shape
    _f32(dz_out, ds_out, dz, ds)
    _u8(masked)
    _i32(start_span)
    _lib.lib().od_latent_perturb_bwd(_p(dz_out), _p(ds_out), _p(masked), _p(start_span), _p(dz), _p(ds), B2, E, l, ds_out.shape[1],
                                     _stream(ds))


def latent_loss_block_frames() -> int:
    return _lib.lib().cdll.od_latent_loss_block_frames()


def latent_loss_ws_floats(B2, L) -> int:
    return _lib.lib().cdll.od_latent_loss_ws_floats(B2, L)


def latent_loss(logits, chart, pred_labels, true_labels, masked, s_reg, loss_ema, ema_init, out, coef, ws, s_reg_weight, training):
    """out[0:11] the components, out[11] s_reg, out[12] the loss; coef[0:11] the gradient coefficients; loss_ema / ema_init (a uint8 view of
    the bool flag) are updated on the device when training."""
    B2, C, L = logits.shape
    _f32(logits, chart, pred_labels, true_labels, s_reg, loss_ema, out, coef, ws)
    _u8(masked, ema_init)
    assert C == 9 and chart.shape == logits.shape and tuple(pred_labels.shape) == tuple(true_labels.shape) == (B2, 5)
    assert masked.numel() == B2 and loss_ema.numel() == 11 and out.numel() >= 13 and coef.numel() >= 11
    _lib.lib().od_latent_loss(_p(logits), _p(chart), _p(pred_labels), _p(true_labels), _p(masked), _p(s_reg), _p(loss_ema), _p(ema_init),
                              _p(out), _p(coef), _p(ws), ws.numel(), B2, L, s_reg_weight, int(training), _stream(logits))


def latent_loss_bwd(logits, chart, pred_labels, true_labels, masked, coef, g, dlogits, dlabels, ds_reg, s_reg_weight):
    B2, _, L = logits.shape
    _f32(logits, chart, pred_labels, true_labels, coef, g, dlogits, dlabels, ds_reg)
    _u8(masked)
    assert dlogits.shape == logits.shape and tuple(dlabels.shape) == (B2, 5)
    _lib.lib().od_latent_loss_bwd(_p(logits), _p(chart), _p(pred_labels), _p(true_labels), _p(masked), _p(coef), _p(g), _p(dlogits),
                                  _p(dlabels), _p(ds_reg), B2, L, s_reg_weight, _stream(logits))


# ---------------------------------------------------------------- latent model, validation over ragged groups (per-map reductions)
def mmd_imq_pairs(s, prior, out, ws):
    """out[g] = (MMD^2, zz, pp, zp) of rows 2g, 2g + 1 of s (2G, S) against the same rows of prior: mmd_imq on each pair, no gradient."""
    N, S = s.shape
    _f32(s, prior, out, ws)
    assert N % 2 == 0 and prior.shape == s.shape and tuple(out.shape) == (N // 2, 4) and ws.numel() >= 3 * N
    _lib.lib().od_mmd_imq_pairs(_p(s), _p(prior), _p(out), _p(ws), ws.numel(), N // 2, S, _stream(s))


def latent_loss_maps(logits, chart, hlens, pred_labels, true_labels, s_reg, loss_ema, out, ws, s_reg_weight):
    """out[g] = the 13 values of latent_loss(training=False) on rows 2g, 2g + 1 of logits / chart (2G, 9, Hmax), each valid for hlens[2g]
    frames (device int32 [2G]); s_reg: fp32 [G] with any element stride (a column of mmd_imq_pairs' output); loss_ema is read only."""
    B2, C, Hmax = logits.shape
    G = B2 // 2
    _f32(logits, chart, pred_labels, true_labels, loss_ema, out, ws)
    _lens(hlens, B2)
    assert C == 9 and B2 % 2 == 0 and chart.shape == logits.shape and tuple(pred_labels.shape) == tuple(true_labels.shape) == (B2, 5)
    assert s_reg.dtype == torch.float32 and s_reg.dim() == 1 and s_reg.shape[0] == G and (G == 1 or s_reg.stride(0) >= 1)
    assert loss_ema.numel() == 11 and tuple(out.shape) == (G, 13)
    _lib.lib().od_latent_loss_maps(_p(logits), _p(chart), _p(hlens), _p(pred_labels), _p(true_labels), _p(s_reg), max(s_reg.stride(0), 1),
                                   _p(loss_ema), _p(out), _p(ws), ws.numel(), G, Hmax, s_reg_weight, _stream(logits))


def latent_eval_maps_ws_floats(G, Pmax) -> int:
    return _lib.lib().cdll.od_latent_eval_maps_ws_floats(G, Pmax)


def latent_eval_maps(chart, pred_chart, plens, z, zlens, pred_labels, true_labels, out, ws):
    """out[g] = (sum t^2, sum p t, sum p^2 on the onset channel; cursor velocity residual and total sums of squares in pixels; mean |pixel
    error|; mean |label error|; min over channels of the unbiased variance of z) of map g: chart / pred_chart (G, 9, Pmax) valid for
    plens[g] frames, z (G, E, lmax) for zlens[g] (device int32 [G] each)."""
    G, C, Pmax = chart.shape
    _f32(chart, pred_chart, z, pred_labels, true_labels, out, ws)
    _lens(plens, G)
    _lens(zlens, G)
    assert C == 9 and pred_chart.shape == chart.shape and z.dim() == 3 and z.shape[0] == G
    assert tuple(pred_labels.shape) == tuple(true_labels.shape) == (G, 5) and tuple(out.shape) == (G, 8)
    _lib.lib().od_latent_eval_maps(_p(chart), _p(pred_chart), _p(plens), _p(z), _p(zlens), _p(pred_labels), _p(true_labels), _p(out), _p(ws),
                                   ws.numel(), G, Pmax, z.shape[1], z.shape[2], _stream(chart))
