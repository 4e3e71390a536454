"""Attention at head_dim 128 — forward, varlen forward and the two-kernel backward — under test_attention_paths.py's own harness: the same
fp64 reference from the rounded operands, the same 64-row blocks, the same input families and the same BOUNDS, imported and not restated.

Dispatch (osu_dreamer_amd/csrc/attn.hip).  No choice depends on the length, so there is no switch length to straddle:

  operands   q_prescaled  kernel                                                 registers / LDS
  bf16       yes          flash_fwd16x_kernel<4, 2, bf16_t, VL, 128>             the 16x16x32 forward templated on the head dim; two waves per SIMD, 64 KiB
  bf16       no           flash_fwd_kernel<bf16_t, 128, OD_ATTN_NW, false, 2>    two waves per SIMD, 64 KiB
  fp32       no / yes     flash_fwd_kernel<float, 128, 4, PRE, 2>                one wave per SIMD (the 128 KiB of LDS leave room for one workgroup)
  fp32 (x3)  no / yes     flash_fwd_kernel<f32x3_t, 128, 4, PRE, 2>              one wave per SIMD
  bf16       no / yes     flash_bwd_dkv_kernel<bf16_t, 128, OD_BWD128_NK, 4> + flash_bwd_dq_kernel<bf16_t, 128, OD_BWD128_NQ, OD_ATTN_NW>
  fp32       no / yes     flash_bwd_dkv_kernel<float, 128, 1, 4> + flash_bwd_dq_kernel<float, 128, 1, 4>      one wave per SIMD

Half operands (OD_F16) and the fused five-pass backward stay head_dim 64 only, and every other head dim is refused: checked at the end.

Shapes: test_attention_paths.py's small ones on both backends (ragged key tiles at L mod 64 in {1, 5, 44, 63}, more than one 128-query workgroup,
two heads, two sequences); on the GPU 1 x 3 x 2049 forward (as head_dim 32 has, and with the pre-multiplied q of the 16x16x32 form) and
1 x 3 x 2047 pair backward.
"""
import math

import pytest
import torch

from osu_dreamer_amd import ops
from osu_dreamer_amd._lib import HipKernelError
from kernel_backend import dev  # noqa: F401
from test_attention_paths import BOUNDS, SMALL_BWD, SMALL_FWD, Case, gpu, run_case  # noqa: F401
from test_varlen_kernels import test_attn_fwd_varlen as attn_fwd_varlen

HD = 128
assert set(BOUNDS) == {"bf16", "f16", "fp32", "x3"}

FWD_CONFIGS_128 = [("bf16", True), ("bf16", False), ("fp32", False), ("fp32", True), ("x3", False)]
SMALL_CASES = [Case(op, HD, pre, fam, *s) for op, pre in FWD_CONFIGS_128 for fam, shapes in SMALL_FWD.items() for s in shapes]
SMALL_CASES += [Case(op, HD, pre, fam, *s, bwd="pair") for op in ("bf16", "fp32") for pre in (False, True) for fam, s in SMALL_BWD]
SMALL_CASES += [Case("bf16", HD, True, "padtrap", 1, 1, 127, bwd="pair"), Case("bf16", HD, True, "padtrap", 1, 1, 65)]

LONG_CASES = [Case(op, HD, False, fam, 1, 3, 2049) for op in ("bf16", "fp32", "x3") for fam in ("random", "padtrap", "peak_moderate", "moving")]
LONG_CASES += [Case("bf16", HD, True, fam, 1, 3, 2049) for fam in ("random", "padtrap", "peak_moderate", "moving", "moving_last")]
LONG_CASES += [Case(op, HD, pre, fam, 1, 3, 2047, bwd="pair") for op in ("bf16", "fp32") for pre in (False, True)
               for fam in ("random", "padtrap", "moving")]


@pytest.mark.parametrize("case", SMALL_CASES, ids=lambda c: c.id)
def test_attention_hd128_small(dev, case):
    run_case(case, dev)


@pytest.mark.gpu
@pytest.mark.parametrize("case", LONG_CASES, ids=lambda c: c.id)
def test_attention_hd128_long(gpu, case):
    run_case(case, gpu)


@pytest.mark.parametrize("op,pre", [("bf16", True), ("fp32", False), ("x3", False)], ids=["bf16-pre", "fp32-raw", "x3-raw"])
def test_attention_hd128_varlen(dev, op, pre):
    attn_fwd_varlen(dev, op, HD, pre)


def _buffers(dtype, B, H, L, hd, device):
    dh = H * hd
    q, k, v, o, do, dq, dk, dv = (torch.zeros(B * L, dh, dtype=dtype, device=device) for _ in range(8))
    lse, delta = torch.zeros(B, H, L, device=device), torch.zeros(B, H, L, device=device)
    return q, k, v, o, do, dq, dk, dv, lse, delta


@pytest.mark.parametrize("hd", [96, 256])
def test_other_head_dims_are_still_refused(dev, hd):
    B, H, L = 1, 1, 64
    sc = 1 / math.sqrt(hd)
    for dtype in (torch.bfloat16, torch.float32):
        q, k, v, o, do, dq, dk, dv, lse, delta = _buffers(dtype, B, H, L, hd, dev)
        with pytest.raises(HipKernelError):
            ops.flash_attn_fwd(q, k, v, o, lse, B, H, L, hd, sc)
        with pytest.raises(HipKernelError):
            ops.flash_attn_fwd_varlen(q, k, v, o, lse, torch.tensor([L], dtype=torch.int32, device=dev), B, H, L, hd, sc)
        with pytest.raises(HipKernelError):
            ops.flash_attn_bwd(q, k, v, o, do, lse, delta, dq, dk, dv, B, H, L, hd, sc)


def test_half_operands_and_the_fused_backward_stay_head_dim_64(dev):
    B, H, L = 1, 1, 64
    sc = 1 / math.sqrt(HD)
    q, k, v, o, do, dq, dk, dv, lse, delta = _buffers(torch.float16, B, H, L, HD, dev)
    ob = o.to(torch.bfloat16)
    with pytest.raises(HipKernelError):
        ops.flash_attn_fwd(q, k, v, ob, lse, B, H, L, HD, sc, q_prescaled=True)
    q, k, v, o, do, dq, dk, dv, lse, delta = _buffers(torch.bfloat16, B, H, L, HD, dev)
    ws = ops.FusedAttnBwdWorkspace(B, H, L, dev, torch.bfloat16)
    with pytest.raises(HipKernelError):
        ops.flash_attn_bwd_fused(q, k, v, o, do, lse, dq, dk, dv, B, H, L, HD, sc, ws, q_prescaled=True)
