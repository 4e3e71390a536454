// Style-model sampler pieces that are not already covered by the denoiser's entry points
// (osu_dreamer/models/style/model.py:73-100).  Everything is fp32 on [B][H] vectors (B = diffs, H = 256).
#include "od_common.h"
#include "od_api_internal.h"

namespace {

// c[b][h] = sum_n ( labels[b][n] < 0 ? null[n][h] : cond_b[n][h] + sum_f rff(b,n,f) * cond_w[n][f][h] ),
// rff(b,n,f) = scale * cos(labels[b][n]/10 * W[f] + bias[f])           — style/model.py:73-80
__global__ __launch_bounds__(256) void style_cond_kernel(const float* __restrict__ labels, const float* __restrict__ rffW,
                                                         const float* __restrict__ rffb, const float* __restrict__ cw,
                                                         const float* __restrict__ cb, const float* __restrict__ nul,
                                                         float* __restrict__ c, int NL, int F, int H, float scale) {
    OD_DYN_SMEM(smem_raw);
    float* s_rff = (float*)smem_raw;       // [NL][F]
    const int b = blockIdx.y;
    for (int i = threadIdx.x; i < NL * F; i += 256) {
        const int n = i / F, f = i % F;
        s_rff[i] = scale * cosf(labels[b * NL + n] / 10.0f * rffW[f] + rffb[f]);
    }
    __syncthreads();
    const int h = blockIdx.x * 256 + threadIdx.x;
    if (h >= H) return;
    float acc = 0.f;
    for (int n = 0; n < NL; n++) {
        if (labels[b * NL + n] < 0.f) { acc += nul[n * H + h]; continue; }
        float s = cb[n * H + h];
        for (int f = 0; f < F; f++) s += s_rff[n * F + f] * cw[((size_t)n * F + f) * H + h];
        acc += s;
    }
    c[(size_t)b * H + h] = acc;
}

// y[m] = x[m] * rsqrt(mean(x[m]^2) + eps) (* gamma)        — nn.RMSNorm / rms_norm on row vectors
__global__ __launch_bounds__(256) void rmsnorm_rows_kernel(const float* __restrict__ x, const float* __restrict__ gamma,
                                                           float* __restrict__ y, int M, int C, float eps) {
    const int lane = threadIdx.x & 63;
    const int m = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (m >= M) return;
    float ss = 0.f;
    for (int c = lane; c < C; c += 64) { const float v = x[(size_t)m * C + c]; ss += v * v; }
    const float inv = rsqrtf(od_wave_sum(ss) / (float)C + eps);
    for (int c = lane; c < C; c += 64) y[(size_t)m * C + c] = x[(size_t)m * C + c] * inv * (gamma ? gamma[c] : 1.f);
}

// Backward of style_cond_kernel (autograd of style/model.py:73-80).  One workgroup owns the tile (label n, SC_FT features, 256 columns h)
// of d cond_w and walks the batch in order, one thread per column with the SC_FT sums in registers: no atomics, the same bits every run.
// The Fourier features are recomputed (the forward's expression) per 64-row slab into LDS.  A masked label (< 0) is skipped by a branch,
// never multiplied by 0: whatever its feature evaluates to (NaN for -inf) is not read.  The f-tile 0 workgroup also owns d cond_b / d null.
constexpr int SC_FT = 16, SC_BS = 64;
__global__ __launch_bounds__(256) void style_cond_bwd_kernel(const float* __restrict__ labels, const float* __restrict__ rffW,
                                                             const float* __restrict__ rffb, const float* __restrict__ dc,
                                                             float* __restrict__ dcw, float* __restrict__ dcb, float* __restrict__ dnul,
                                                             int B, int NL, int F, int H, float scale) {
    __shared__ float s_rff[SC_BS][SC_FT];
    __shared__ float s_lab[SC_BS];
    const int n = blockIdx.y, f0 = blockIdx.z * SC_FT;
    const int h = blockIdx.x * 256 + threadIdx.x;
    float acc[SC_FT];
#pragma unroll
    for (int i = 0; i < SC_FT; i++) acc[i] = 0.f;
    float sb = 0.f, sn = 0.f;
    for (int b0 = 0; b0 < B; b0 += SC_BS) {
        const int nb = B - b0 < SC_BS ? B - b0 : SC_BS;
        for (int i = threadIdx.x; i < SC_BS * SC_FT; i += 256) {
            const int bl = i / SC_FT, fl = i % SC_FT;
            float r = 0.f;
            if (bl < nb && f0 + fl < F) {
                const float lab = labels[(size_t)(b0 + bl) * NL + n];
                if (!(lab < 0.f)) r = scale * cosf(lab / 10.0f * rffW[f0 + fl] + rffb[f0 + fl]);
            }
            s_rff[bl][fl] = r;
        }
        if (threadIdx.x < SC_BS) s_lab[threadIdx.x] = threadIdx.x < nb ? labels[(size_t)(b0 + threadIdx.x) * NL + n] : 0.f;
        __syncthreads();
        if (h < H) {
            for (int bl = 0; bl < nb; bl++) {
                const float g = dc[(size_t)(b0 + bl) * H + h];
                if (s_lab[bl] < 0.f) { sn += g; continue; }
                sb += g;
#pragma unroll
                for (int i = 0; i < SC_FT; i++) acc[i] += s_rff[bl][i] * g;
            }
        }
        __syncthreads();
    }
    if (h >= H) return;
#pragma unroll
    for (int i = 0; i < SC_FT; i++)
        if (f0 + i < F) dcw[((size_t)n * F + f0 + i) * H + h] += acc[i];
    if (blockIdx.z == 0) { dcb[n * H + h] += sb; dnul[n * H + h] += sn; }
}

// Backward of rmsnorm_rows_kernel: with xhat = x * inv and g = dy * gamma,  dx (+)= inv * (g - xhat * mean_c(g * xhat)).  One wave per row.
__global__ __launch_bounds__(256) void rmsnorm_rows_bwd_dx_kernel(const float* __restrict__ x, const float* __restrict__ gamma,
                                                                  const float* __restrict__ dy, float* __restrict__ dx, int M, int C,
                                                                  float eps, int accumulate) {
    const int lane = threadIdx.x & 63;
    const int m = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (m >= M) return;
    float ss = 0.f, gx = 0.f;
    for (int c = lane; c < C; c += 64) {
        const float v = x[(size_t)m * C + c];
        ss += v * v;
        gx += dy[(size_t)m * C + c] * (gamma ? gamma[c] : 1.f) * v;
    }
    const float inv = rsqrtf(od_wave_sum(ss) / (float)C + eps);
    const float k = od_wave_sum(gx) * inv * inv / (float)C;       // mean_c(g * xhat) * inv
    for (int c = lane; c < C; c += 64) {
        const size_t i = (size_t)m * C + c;
        const float d = inv * (dy[i] * (gamma ? gamma[c] : 1.f) - x[i] * k);
        dx[i] = accumulate ? dx[i] + d : d;
    }
}

// dgamma[c] += sum_m dy[m][c] * xhat[m][c]: one workgroup owns 256 columns and walks the rows in order (no atomics, the same bits every
// run); per 64-row slab its four waves first recompute the rows' inv_rms into LDS.
__global__ __launch_bounds__(256) void rmsnorm_rows_bwd_dgamma_kernel(const float* __restrict__ x, const float* __restrict__ dy,
                                                                      float* __restrict__ dgamma, int M, int C, float eps) {
    __shared__ float s_inv[64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int c = blockIdx.x * 256 + threadIdx.x;
    float acc = 0.f;
    for (int m0 = 0; m0 < M; m0 += 64) {
        const int nm = M - m0 < 64 ? M - m0 : 64;
        for (int r = wave; r < nm; r += 4) {
            float ss = 0.f;
            for (int cc = lane; cc < C; cc += 64) { const float v = x[(size_t)(m0 + r) * C + cc]; ss += v * v; }
            ss = od_wave_sum(ss);
            if (lane == 0) s_inv[r] = rsqrtf(ss / (float)C + eps);
        }
        __syncthreads();
        if (c < C)
            for (int r = 0; r < nm; r++) acc += dy[(size_t)(m0 + r) * C + c] * x[(size_t)(m0 + r) * C + c] * s_inv[r];
        __syncthreads();
    }
    if (c < C) dgamma[c] += acc;
}

// dst[i] = (TD)src[i]: the fp32 <-> bf16 boundary of the bf16 training step (fp32 narrow linears and heads either side of bf16 GEMM blocks)
template <class TS, class TD>
__global__ __launch_bounds__(256) void cast_rows_kernel(const TS* __restrict__ src, TD* __restrict__ dst, long n) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i < n) od_t<TD>::st(dst + i, od_t<TS>::ld(src + i));
}

}  // namespace

extern "C" int od_style_conditioning(const float* labels, const float* rff_w, const float* rff_b, const float* cond_w,
                                     const float* cond_b, const float* null_labels, float* c, int B, int NL, int F, int H,
                                     void* stream) {
    if (NL * F * 4 > 60000) return OD_ERR_UNSUPPORTED;
    const float scale = sqrtf(2.0f / (float)F);
    OD_LAUNCH(style_cond_kernel, dim3((H + 255) / 256, B), dim3(256), NL * F * sizeof(float), (hipStream_t)stream, labels, rff_w, rff_b,
              cond_w, cond_b, null_labels, c, NL, F, H, scale);
    OD_CHECK_LAUNCH();
    return 0;
}

extern "C" int od_rmsnorm_rows(const float* x, const float* gamma, float* y, int M, int C, float eps, void* stream) {
    OD_LAUNCH(rmsnorm_rows_kernel, dim3((M + 3) / 4), dim3(256), 0, (hipStream_t)stream, x, gamma, y, M, C, eps);
    OD_CHECK_LAUNCH();
    return 0;
}

extern "C" int od_style_conditioning_bwd(const float* labels, const float* rff_w, const float* rff_b, const float* dc, float* dcond_w,
                                         float* dcond_b, float* dnull_labels, int B, int NL, int F, int H, void* stream) {
    if (B <= 0 || NL <= 0 || F <= 0 || H <= 0 || !dcond_w || !dcond_b || !dnull_labels) return OD_ERR_ARG;
    const float scale = sqrtf(2.0f / (float)F);
    OD_LAUNCH(style_cond_bwd_kernel, dim3((H + 255) / 256, NL, (F + SC_FT - 1) / SC_FT), dim3(256), 0, (hipStream_t)stream, labels, rff_w,
              rff_b, dc, dcond_w, dcond_b, dnull_labels, B, NL, F, H, scale);
    OD_CHECK_LAUNCH();
    return 0;
}

extern "C" int od_rmsnorm_rows_bwd(const float* x, const float* gamma, const float* dy, float* dx, float* dgamma, int M, int C, float eps,
                                   int accumulate_dx, void* stream) {
    if (M <= 0 || C <= 0 || !dx || (dgamma && !gamma)) return OD_ERR_ARG;
    OD_LAUNCH(rmsnorm_rows_bwd_dx_kernel, dim3((M + 3) / 4), dim3(256), 0, (hipStream_t)stream, x, gamma, dy, dx, M, C, eps, accumulate_dx);
    if (dgamma)
        OD_LAUNCH(rmsnorm_rows_bwd_dgamma_kernel, dim3((C + 255) / 256), dim3(256), 0, (hipStream_t)stream, x, dy, dgamma, M, C, eps);
    OD_CHECK_LAUNCH();
    return 0;
}

extern "C" int od_cast_rows(int src_dtype, const void* src, int dst_dtype, void* dst, long n, void* stream) {
    if (n <= 0 || !src || !dst) return OD_ERR_ARG;
    const dim3 grid((unsigned)((n + 255) / 256));
    if (src_dtype == OD_F32 && dst_dtype == OD_BF16)
        OD_LAUNCH((cast_rows_kernel<float, bf16_t>), grid, dim3(256), 0, (hipStream_t)stream, (const float*)src, (bf16_t*)dst, n);
    else if (src_dtype == OD_BF16 && dst_dtype == OD_F32)
        OD_LAUNCH((cast_rows_kernel<bf16_t, float>), grid, dim3(256), 0, (hipStream_t)stream, (const bf16_t*)src, (float*)dst, n);
    else return OD_ERR_UNSUPPORTED;
    OD_CHECK_LAUNCH();
    return 0;
}
