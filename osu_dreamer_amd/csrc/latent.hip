// Latent model (osu_dreamer/models/latent/{spec_features,unet,model}.py): the inference path, the step either
// side of diffusion.sample in LDM.sample, and (second half of the file) the backward kernels of the same calls.
// Frame-major [B*L][C] like the denoiser; C = h_dim = 128 is narrower than a wavefront x 8 channels, so here
// G = C/8 lanes own a frame and a wave walks 64/G frames.
// The SwiGLU body of each block reuses od_dwconv / od_gemm_nt / od_swiglu_rmsnorm.  All HBM-bound row work.
// VL forms (several songs / maps of different lengths in one call): sequence b of the padded [B*L][C] layout is valid for frames
// < lens[b] (device int32 [B], the lengths AT THE LEVEL the kernel reads); taps and frames past it read as zero, selected, never
// multiplied by 0 (padding may hold NaN), and frames past it that a kernel hands back are written as exact zeros.
#include "od_common.h"
#include "od_api_internal.h"

namespace {

__device__ __forceinline__ float group_sum(float v, int G) {
    for (int m = G >> 1; m >= 1; m >>= 1) v += __shfl_xor(v, m);
    return v;
}
__device__ __forceinline__ float sumsq8(const float (&v)[8]) {
    float s = 0.f;
#pragma unroll
    for (int e = 0; e < 8; e++) s += v[e] * v[e];
    return s;
}
// frame and channel owned by this lane: G lanes per frame, 256/G frames per block
#define OD_ROW_OF_LANE()                                                        \
    const int G = C >> 3;                                                       \
    const long m = (long)blockIdx.x * (256 / G) + threadIdx.x / G;              \
    const int c = (threadIdx.x % G) * 8;                                        \
    const bool live = m < M;                                                    \
    const long mr = live ? m : M - 1   /* dead lanes shadow the last frame so shuffles stay convergent */

// y = act( rms_norm(x) * gamma * (1 + scale[b]) + shift[b] )       unet.py:50 (norm + FiLM), :51 out_norm,
//                                                                  spec_features.py:27-28 (norm + SiLU)
// VL: frames l >= lens[b] are written as 0.
template <class T, bool VL = false>
__global__ __launch_bounds__(256) void rms_affine_film_kernel(const T* __restrict__ x, int ldx, const float* __restrict__ gamma,
                                                              const float* __restrict__ ssg, T* __restrict__ y, int ldy,
                                                              long M, int L, int C, float eps, int act,
                                                              const int* __restrict__ lens = nullptr) {
    OD_ROW_OF_LANE();
    float v[8], g[8], o[8];
    od_ld8(x + mr * ldx + c, v);
    const float inv = rsqrtf(group_sum(sumsq8(v), G) / (float)C + eps);
    od_ld8(gamma + c, g);
#pragma unroll
    for (int e = 0; e < 8; e++) o[e] = v[e] * inv * g[e];
    if (ssg) {
        const float* sc = ssg + (size_t)(mr / L) * 3 * C;
        float s[8], sh[8];
        od_ld8(sc + c, s); od_ld8(sc + C + c, sh);
#pragma unroll
        for (int e = 0; e < 8; e++) o[e] = o[e] * (1.f + s[e]) + sh[e];
    }
    if (act == OD_ACT_SILU) {
#pragma unroll
        for (int e = 0; e < 8; e++) o[e] = od_silu(o[e]);
    }
    if (VL && (int)(mr % L) >= lens[mr / L]) {
#pragma unroll
        for (int e = 0; e < 8; e++) o[e] = 0.f;
    }
    if (live) od_st8(y + m * ldy + c, o);
}

// xo = x + rms_norm(h) * gamma * (1 + gate[b])                      unet.py:28,51
template <class T>
__global__ __launch_bounds__(256) void rms_affine_gate_res_kernel(const T* __restrict__ x, int ldx, const T* __restrict__ h, int ldh,
                                                                  const float* __restrict__ gamma, const float* __restrict__ ssg,
                                                                  T* __restrict__ xo, int ldxo, long M, int L, int C, float eps) {
    OD_ROW_OF_LANE();
    float v[8], g[8], r[8], o[8];
    od_ld8(h + mr * ldh + c, v);
    const float inv = rsqrtf(group_sum(sumsq8(v), G) / (float)C + eps);
    od_ld8(gamma + c, g);
    od_ld8(x + mr * ldx + c, r);
    float gt[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    if (ssg) od_ld8(ssg + (size_t)(mr / L) * 3 * C + 2 * C + c, gt);
#pragma unroll
    for (int e = 0; e < 8; e++) o[e] = r[e] + v[e] * inv * g[e] * (1.f + gt[e]);
    if (live) od_st8(xo + m * ldxo + c, o);
}

// xo = x + rms_norm(p) * gamma * gx;  p = proj(skip) rows (frame l of batch 0 when the skip is broadcast),
// gx = gate(x) rows                                                 unet.py:117-126 (mixer)
// VL: row b reads frame l of skip row prow[b] (several decoder rows per song share that song's skip); p_bcast is ignored.
template <class T, bool VL = false>
__global__ __launch_bounds__(256) void mixer_kernel(const T* __restrict__ x, int ldx, const T* __restrict__ p, int ldp, int p_bcast,
                                                    const T* __restrict__ gx, int ldg, const float* __restrict__ gamma,
                                                    T* __restrict__ xo, int ldxo, long M, int L, int C, float eps,
                                                    const int* __restrict__ prow = nullptr) {
    OD_ROW_OF_LANE();
    float v[8], g[8], r[8], q[8], o[8];
    const long pr = VL ? (long)prow[mr / L] * L + mr % L : (p_bcast ? mr % L : mr);
    od_ld8(p + pr * ldp + c, v);
    const float inv = rsqrtf(group_sum(sumsq8(v), G) / (float)C + eps);
    od_ld8(gamma + c, g);
    od_ld8(x + mr * ldx + c, r);
    od_ld8(gx + mr * ldg + c, q);
#pragma unroll
    for (int e = 0; e < 8; e++) o[e] = r[e] + v[e] * inv * g[e] * q[e];
    if (live) od_st8(xo + m * ldxo + c, o);
}

// y[b][lo][c] = mean_{j<s} ( bias[c] + sum_k w[c][k] x[b][s*lo + j + k - r][c] ),  k = 2r+1 = 1 + 2*(s/2), zero padded
// — depthwise conv then AvgPool1d(s)                                unet.py:58-63
// VL: input frames >= lens[b] (input level) read as zero; outputs lo >= lens[b] / s are written as 0.
template <class T, bool VL = false>
__global__ __launch_bounds__(256) void unet_down_kernel(const T* __restrict__ x, int ldx, const float* __restrict__ w,
                                                        const float* __restrict__ bias, T* __restrict__ y, int ldy, int B, int Lo,
                                                        int C, int s, const int* __restrict__ lens = nullptr) {
    const int G = C >> 3, r = s / 2, ks = 2 * r + 1, L = Lo * s;
    const long M = (long)B * Lo;
    const long m = (long)blockIdx.x * (256 / G) + threadIdx.x / G;
    const int c = (threadIdx.x % G) * 8;
    if (m >= M) return;
    const int b = (int)(m / Lo), lo = (int)(m % Lo);
    const int Lv = VL ? (lens[b] < L ? lens[b] : L) : L;      // (clamped: a bad length never reads past the sequence)
    float acc[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    // sum_j sum_k w[k] x[s*lo + j + k - r]  =  sum_t x[s*lo - r + t] * (sum of w[k] over k + j = t)
    for (int t = 0; t < s + ks - 1; t++) {
        const int l = s * lo - r + t;
        if (l < 0 || l >= Lv) continue;
        float v[8];
        od_ld8(x + ((long)b * L + l) * ldx + c, v);
        const int k0 = t - (s - 1) > 0 ? t - (s - 1) : 0, k1 = t < ks - 1 ? t : ks - 1;
#pragma unroll
        for (int e = 0; e < 8; e++) {
            float ws = 0.f;
            for (int k = k0; k <= k1; k++) ws += w[(c + e) * ks + k];
            acc[e] += ws * v[e];
        }
    }
    float bb[8], o[8];
    od_ld8(bias + c, bb);
#pragma unroll
    for (int e = 0; e < 8; e++) o[e] = (VL && lo >= Lv / s) ? 0.f : acc[e] / (float)s + bb[e];
    od_st8(y + m * ldy + c, o);
}

// y[b][l][c] = bias[c] + sum_k w[c][k] x[b][(l + k - r) / s][c] for 0 <= l + k - r < s*Li
// — nearest Upsample(s) then depthwise conv                          unet.py:80-85
// VL: sequence b is lens[b] frames long at the input level, s*lens[b] at the output: taps at lu >= s*lens[b] read as zero,
// outputs there are written as 0.
template <class T, bool VL = false>
__global__ __launch_bounds__(256) void unet_up_kernel(const T* __restrict__ x, int ldx, const float* __restrict__ w,
                                                      const float* __restrict__ bias, T* __restrict__ y, int ldy, int B, int Li,
                                                      int C, int s, const int* __restrict__ lens = nullptr) {
    const int G = C >> 3, r = s / 2, ks = 2 * r + 1, L = Li * s;
    const long M = (long)B * L;
    const long m = (long)blockIdx.x * (256 / G) + threadIdx.x / G;
    const int c = (threadIdx.x % G) * 8;
    if (m >= M) return;
    const int b = (int)(m / L), l = (int)(m % L);
    const int Lv = VL ? s * (lens[b] < Li ? lens[b] : Li) : L;
    float o[8];
    od_ld8(bias + c, o);
    for (int k = 0; k < ks; k++) {
        const int lu = l + k - r;
        if (lu < 0 || lu >= Lv) continue;
        float v[8];
        od_ld8(x + ((long)b * Li + lu / s) * ldx + c, v);
#pragma unroll
        for (int e = 0; e < 8; e++) o[e] += w[(c + e) * ks + k] * v[e];
    }
    if (VL && l >= Lv) {
#pragma unroll
        for (int e = 0; e < 8; e++) o[e] = 0.f;
    }
    od_st8(y + m * ldy + c, o);
}

// out[b][n][l] = f_n( bias[n] + sum_c W[n][c] x[(b,l)][c] ),  f_n = sigmoid for n < n_sigmoid, identity after;
// with rms != 0 the N outputs of a frame are RMS-normalised (no gain) instead
// — proj_out + the hit-signal sigmoid of decode (latent/model.py:114,127-131); temporal_head (:65-68)
// VL: frames l >= lens[b] are written as 0 (both modes).
template <class T, int NMAX, bool VL = false>
__global__ __launch_bounds__(256) void chart_head_kernel(const T* __restrict__ x, int ldx, const float* __restrict__ W,
                                                         const float* __restrict__ bias, float* __restrict__ out, long M, int L,
                                                         int C, int N, int n_sigmoid, int rms, float eps,
                                                         const int* __restrict__ lens = nullptr) {
    OD_ROW_OF_LANE();
    float v[8];
    od_ld8(x + mr * ldx + c, v);
    const int b = (int)(mr / L), l = (int)(mr % L);
    float y[NMAX], ss = 0.f;
#pragma unroll
    for (int n = 0; n < NMAX; n++) {
        y[n] = 0.f;
        if (n >= N) continue;
        float wv[8], s = 0.f;
        od_ld8(W + (size_t)n * C + c, wv);
#pragma unroll
        for (int e = 0; e < 8; e++) s += wv[e] * v[e];
        s = group_sum(s, G) + bias[n];
        if (n < n_sigmoid) s = od_sigmoid(s);
        y[n] = s; ss += s * s;
    }
    const float k = rms ? rsqrtf(ss / (float)N + eps) : 1.f;
    const bool pad = VL && l >= lens[b];
#pragma unroll
    for (int n = 0; n < NMAX; n++)
        if (n < N && live && c == 0) out[((size_t)b * N + n) * L + l] = pad ? 0.f : y[n] * k;
}

// AttnPool (latent/model.py:23-36): out[b][h*hd + d] = sum_l softmax_l(scores[(b,l)][h]) * values[(b,l)][h*hd + d].
// One block per (b, h); thread = feature d (hd <= 256), softmax statistics by a block reduction over the frames.
// VL: softmax and sum over the frames l < lens[b] of sequence b only (L stays the stride); lens[b] <= 0 gives 0, not 0/0.
template <class T, bool VL = false>
__global__ __launch_bounds__(256) void attn_pool_kernel(const T* __restrict__ scores, int lds_, const T* __restrict__ values, int ldv,
                                                        float* __restrict__ out, int L, int Hh, int hd,
                                                        const int* __restrict__ lens = nullptr) {
    __shared__ float red[256];
    __shared__ float s_p[256];
    const int b = blockIdx.y, h = blockIdx.x, t = threadIdx.x;
    const int Lv = VL ? od_uniform(lens[b] < L ? lens[b] : L) : L;
    const T* sb = scores + (size_t)b * L * lds_ + h;
    float mx = -3.0e38f;
    for (int l = t; l < Lv; l += 256) mx = fmaxf(mx, od_t<T>::ld(sb + (size_t)l * lds_));
    red[t] = mx;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) { if (t < s) red[t] = fmaxf(red[t], red[t + s]); __syncthreads(); }
    mx = red[0];
    __syncthreads();
    float acc = 0.f, den = 0.f;
    for (int l0 = 0; l0 < Lv; l0 += 256) {
        const int l = l0 + t;
        s_p[t] = l < Lv ? __expf(od_t<T>::ld(sb + (size_t)l * lds_) - mx) : 0.f;
        __syncthreads();
        const int n = Lv - l0 < 256 ? Lv - l0 : 256;
        if (t < hd) {
            const T* vb = values + ((size_t)b * L + l0) * ldv + h * hd + t;
            for (int j = 0; j < n; j++) acc += s_p[j] * od_t<T>::ld(vb + (size_t)j * ldv);
        }
        for (int j = 0; j < n; j++) den += s_p[j];       // every thread keeps the same denominator
        __syncthreads();
    }
    if (t < hd) out[(size_t)b * Hh * hd + h * hd + t] = (VL && Lv <= 0) ? 0.f : acc / den;   // (VL: an empty sequence pools to 0)
}

// ---- SpecFeatures front end (spec_features.py:17-26): two strided Conv2d over (freq, time), each followed by a
// channel RMS norm (gamma) and SiLU, then 'b c a l -> b (c a) l'.  One block = TL frames; the spectrogram tile
// (with its 2-frame halo and 1-bin zero border) and the first conv's output live in LDS; weights are read with
// wave-uniform indices (scalar loads).
// VL: sequence b is lens[b] frames long (L stays the stride): the input halo and conv2's time padding of h1 end at lens[b], and
// output frames >= lens[b] are written as 0 (a block wholly past lens[b] writes its zeros and leaves).
constexpr int SF_TL = 64, SF_F = 72, SF_C1 = 8, SF_A1 = 12, SF_C2 = 32, SF_A2 = 3;
template <class T, bool VL = false>
__global__ __launch_bounds__(256) void spec_conv_kernel(const float* __restrict__ audio, const float* __restrict__ w1,
                                                        const float* __restrict__ b1, const float* __restrict__ g1,
                                                        const float* __restrict__ w2, const float* __restrict__ b2,
                                                        const float* __restrict__ g2, T* __restrict__ out, int ldo, int L,
                                                        float eps, const int* __restrict__ lens = nullptr) {
    __shared__ float s_in[SF_F + 2][SF_TL + 4];            // freq rows -1..72, frames l0-2 .. l0+TL+1
    __shared__ float s_h1[SF_C1][SF_A1 + 2][SF_TL + 2];    // freq rows -1..12, frames l0-1 .. l0+TL
    const int b = blockIdx.y, l0 = blockIdx.x * SF_TL, tid = threadIdx.x;
    const int Lv = VL ? od_uniform(lens[b] < L ? lens[b] : L) : L;
    if (VL && l0 >= Lv) {
        for (int i = tid; i < SF_A2 * SF_TL; i += 256) {
            const int a = i / SF_TL, l = l0 + i % SF_TL;
            if (l < L) {
#pragma unroll
                for (int c2 = 0; c2 < SF_C2; c2++) od_t<T>::st(out + ((size_t)b * L + l) * ldo + c2 * SF_A2 + a, 0.f);
            }
        }
        return;
    }
    const float* ab = audio + (size_t)b * SF_F * L;
    for (int i = tid; i < (SF_F + 2) * (SF_TL + 4); i += 256) {
        const int f = i / (SF_TL + 4) - 1, t = i % (SF_TL + 4), l = l0 - 2 + t;
        s_in[f + 1][t] = (f >= 0 && f < SF_F && l >= 0 && l < Lv) ? ab[(size_t)f * L + l] : 0.f;
    }
    for (int i = tid; i < SF_C1 * 2 * (SF_TL + 2); i += 256) {   // zero freq border of h1
        const int cc = i / (2 * (SF_TL + 2)), rr = (i / (SF_TL + 2)) % 2, t = i % (SF_TL + 2);
        s_h1[cc][rr ? SF_A1 + 1 : 0][t] = 0.f;
    }
    __syncthreads();
    // conv1 (1 -> 8, kernel (8,3), stride (6,1), pad (1,1)) + rms over the 8 channels + SiLU
    for (int i = tid; i < SF_A1 * (SF_TL + 2); i += 256) {
        const int a = i / (SF_TL + 2), t = i % (SF_TL + 2), l = l0 - 1 + t;
        float acc[SF_C1];
#pragma unroll
        for (int cc = 0; cc < SF_C1; cc++) acc[cc] = b1[cc];
        for (int fi = 0; fi < 8; fi++)
#pragma unroll
            for (int j = 0; j < 3; j++) {
                const float v = s_in[6 * a + fi][t + j];     // freq 6a + fi - 1 (+1 border), frame l + j - 1
#pragma unroll
                for (int cc = 0; cc < SF_C1; cc++) acc[cc] += w1[(cc * 8 + fi) * 3 + j] * v;
            }
        float ss = 0.f;
#pragma unroll
        for (int cc = 0; cc < SF_C1; cc++) ss += acc[cc] * acc[cc];
        const float inv = rsqrtf(ss / (float)SF_C1 + eps);
        const bool inside = l >= 0 && l < Lv;                // conv2 zero-pads h1 in time
#pragma unroll
        for (int cc = 0; cc < SF_C1; cc++) s_h1[cc][a + 1][t] = inside ? od_silu(acc[cc] * inv * g1[cc]) : 0.f;
    }
    __syncthreads();
    // conv2 (8 -> 32, kernel (6,3), stride (4,1), pad (1,1)) + rms over the 32 channels + SiLU
    for (int i = tid; i < SF_A2 * SF_TL; i += 256) {
        const int a = i / SF_TL, t = i % SF_TL, l = l0 + t;
        if (l >= L) continue;
        if (VL && l >= Lv) {
            T* orow = out + ((size_t)b * L + l) * ldo;
#pragma unroll
            for (int c2 = 0; c2 < SF_C2; c2++) od_t<T>::st(orow + c2 * SF_A2 + a, 0.f);
            continue;
        }
        float acc[SF_C2];
#pragma unroll
        for (int c2 = 0; c2 < SF_C2; c2++) acc[c2] = b2[c2];
#pragma unroll 1
        for (int cc = 0; cc < SF_C1; cc++)
#pragma unroll 1
            for (int fi = 0; fi < 6; fi++)
#pragma unroll
                for (int j = 0; j < 3; j++) {
                    const float v = s_h1[cc][4 * a + fi][t + j];   // freq 4a + fi - 1 (+1 border), frame l + j - 1
#pragma unroll
                    for (int c2 = 0; c2 < SF_C2; c2++) acc[c2] += w2[((c2 * SF_C1 + cc) * 6 + fi) * 3 + j] * v;
                }
        float ss = 0.f;
#pragma unroll
        for (int c2 = 0; c2 < SF_C2; c2++) ss += acc[c2] * acc[c2];
        const float inv = rsqrtf(ss / (float)SF_C2 + eps);
        T* orow = out + ((size_t)b * L + l) * ldo;
#pragma unroll
        for (int c2 = 0; c2 < SF_C2; c2++) od_t<T>::st(orow + c2 * SF_A2 + a, od_silu(acc[c2] * inv * g2[c2]));
    }
}

#define DISPATCH_T(DT, CALL)                                       \
    do {                                                           \
        if ((DT) == OD_BF16) { typedef bf16_t T_; CALL; }          \
        else if ((DT) == OD_F32) { typedef float T_; CALL; }       \
        else return OD_ERR_ARG;                                    \
    } while (0)

inline bool lanes_ok(int C) { return C >= 8 && C <= 512 && (C & (C - 1)) == 0; }   // G = C/8 a power of two <= 64
inline unsigned row_grid(long M, int C) { const int rpb = 256 / (C >> 3); return (unsigned)((M + rpb - 1) / rpb); }

}  // namespace

extern "C" int od_spec_features_conv(int dtype, const float* audio, const float* w1, const float* b1, const float* g1,
                                     const float* w2, const float* b2, const float* g2, void* out, int ldo, int B, int F, int L,
                                     float eps, void* stream) {
    if (F != SF_F) return OD_ERR_UNSUPPORTED;
    if (B <= 0 || L <= 0) return OD_ERR_ARG;
    dim3 grid((L + SF_TL - 1) / SF_TL, B);
    DISPATCH_T(dtype, OD_LAUNCH((spec_conv_kernel<T_>), grid, dim3(256), 0, (hipStream_t)stream, audio, w1, b1, g1, w2, b2, g2,
                                (T_*)out, ldo, L, eps));
    OD_CHECK_LAUNCH();
    return 0;
}

extern "C" int od_spec_features_conv_varlen(int dtype, const float* audio, const float* w1, const float* b1, const float* g1,
                                            const float* w2, const float* b2, const float* g2, void* out, int ldo, const int* lens,
                                            int B, int F, int L, float eps, void* stream) {
    if (F != SF_F) return OD_ERR_UNSUPPORTED;
    if (B <= 0 || L <= 0 || !lens) return OD_ERR_ARG;
    dim3 grid((L + SF_TL - 1) / SF_TL, B);
    DISPATCH_T(dtype, OD_LAUNCH((spec_conv_kernel<T_, true>), grid, dim3(256), 0, (hipStream_t)stream, audio, w1, b1, g1, w2, b2, g2,
                                (T_*)out, ldo, L, eps, lens));
    OD_CHECK_LAUNCH();
    return 0;
}

extern "C" int od_rmsnorm_affine_film(int dtype, const void* x, int ldx, const float* gamma, const float* ssg, void* y, int ldy,
                                      int B, int L, int C, float eps, int act, void* stream) {
    if (!lanes_ok(C) || ldx % 8 || ldy % 8) return OD_ERR_ALIGN;
    const long M = (long)B * L;
    DISPATCH_T(dtype, OD_LAUNCH((rms_affine_film_kernel<T_>), dim3(row_grid(M, C)), dim3(256), 0, (hipStream_t)stream, (const T_*)x,
                                ldx, gamma, ssg, (T_*)y, ldy, M, L, C, eps, act));
    OD_CHECK_LAUNCH();
    return 0;
}

extern "C" int od_rmsnorm_affine_film_varlen(int dtype, const void* x, int ldx, const float* gamma, const float* ssg, void* y, int ldy,
                                             const int* lens, int B, int L, int C, float eps, int act, void* stream) {
    if (!lanes_ok(C) || ldx % 8 || ldy % 8) return OD_ERR_ALIGN;
    if (!lens) return OD_ERR_ARG;
    const long M = (long)B * L;
    DISPATCH_T(dtype, OD_LAUNCH((rms_affine_film_kernel<T_, true>), dim3(row_grid(M, C)), dim3(256), 0, (hipStream_t)stream,
                                (const T_*)x, ldx, gamma, ssg, (T_*)y, ldy, M, L, C, eps, act, lens));
    OD_CHECK_LAUNCH();
    return 0;
}

extern "C" int od_rmsnorm_affine_gate_residual(int dtype, const void* x, int ldx, const void* h, int ldh, const float* gamma,
                                               const float* ssg, void* xo, int ldxo, int B, int L, int C, float eps,
                                               void* stream) {
    if (!lanes_ok(C) || ldx % 8 || ldh % 8 || ldxo % 8) return OD_ERR_ALIGN;
    const long M = (long)B * L;
    DISPATCH_T(dtype, OD_LAUNCH((rms_affine_gate_res_kernel<T_>), dim3(row_grid(M, C)), dim3(256), 0, (hipStream_t)stream,
                                (const T_*)x, ldx, (const T_*)h, ldh, gamma, ssg, (T_*)xo, ldxo, M, L, C, eps));
    OD_CHECK_LAUNCH();
    return 0;
}

extern "C" int od_unet_mixer(int dtype, const void* x, int ldx, const void* p, int ldp, int p_bcast, const void* gx, int ldg,
                             const float* gamma, void* xo, int ldxo, int B, int L, int C, float eps, void* stream) {
    if (!lanes_ok(C) || ldx % 8 || ldp % 8 || ldg % 8 || ldxo % 8) return OD_ERR_ALIGN;
    const long M = (long)B * L;
    DISPATCH_T(dtype, OD_LAUNCH((mixer_kernel<T_>), dim3(row_grid(M, C)), dim3(256), 0, (hipStream_t)stream, (const T_*)x, ldx,
                                (const T_*)p, ldp, p_bcast, (const T_*)gx, ldg, gamma, (T_*)xo, ldxo, M, L, C, eps));
    OD_CHECK_LAUNCH();
    return 0;
}

extern "C" int od_unet_mixer_varlen(int dtype, const void* x, int ldx, const void* p, int ldp, const int* prow, const void* gx, int ldg,
                                    const float* gamma, void* xo, int ldxo, int B, int L, int C, float eps, void* stream) {
    if (!lanes_ok(C) || ldx % 8 || ldp % 8 || ldg % 8 || ldxo % 8) return OD_ERR_ALIGN;
    if (!prow) return OD_ERR_ARG;
    const long M = (long)B * L;
    DISPATCH_T(dtype, OD_LAUNCH((mixer_kernel<T_, true>), dim3(row_grid(M, C)), dim3(256), 0, (hipStream_t)stream, (const T_*)x, ldx,
                                (const T_*)p, ldp, 0, (const T_*)gx, ldg, gamma, (T_*)xo, ldxo, M, L, C, eps, prow));
    OD_CHECK_LAUNCH();
    return 0;
}

extern "C" int od_unet_down(int dtype, const void* x, int ldx, const float* w, const float* bias, void* y, int ldy, int B, int Lo,
                            int C, int stride, void* stream) {
    if (!lanes_ok(C) || ldx % 8 || ldy % 8) return OD_ERR_ALIGN;
    if (stride < 1 || stride > 8) return OD_ERR_UNSUPPORTED;
    const long M = (long)B * Lo;
    DISPATCH_T(dtype, OD_LAUNCH((unet_down_kernel<T_>), dim3(row_grid(M, C)), dim3(256), 0, (hipStream_t)stream, (const T_*)x, ldx,
                                w, bias, (T_*)y, ldy, B, Lo, C, stride));
    OD_CHECK_LAUNCH();
    return 0;
}

extern "C" int od_unet_down_varlen(int dtype, const void* x, int ldx, const float* w, const float* bias, void* y, int ldy, const int* lens,
                                   int B, int Lo, int C, int stride, void* stream) {
    if (!lanes_ok(C) || ldx % 8 || ldy % 8) return OD_ERR_ALIGN;
    if (stride < 1 || stride > 8) return OD_ERR_UNSUPPORTED;
    if (!lens) return OD_ERR_ARG;
    const long M = (long)B * Lo;
    DISPATCH_T(dtype, OD_LAUNCH((unet_down_kernel<T_, true>), dim3(row_grid(M, C)), dim3(256), 0, (hipStream_t)stream, (const T_*)x,
                                ldx, w, bias, (T_*)y, ldy, B, Lo, C, stride, lens));
    OD_CHECK_LAUNCH();
    return 0;
}

extern "C" int od_unet_up(int dtype, const void* x, int ldx, const float* w, const float* bias, void* y, int ldy, int B, int Li,
                          int C, int stride, void* stream) {
    if (!lanes_ok(C) || ldx % 8 || ldy % 8) return OD_ERR_ALIGN;
    if (stride < 1 || stride > 8) return OD_ERR_UNSUPPORTED;
    const long M = (long)B * Li * stride;
    DISPATCH_T(dtype, OD_LAUNCH((unet_up_kernel<T_>), dim3(row_grid(M, C)), dim3(256), 0, (hipStream_t)stream, (const T_*)x, ldx, w,
                                bias, (T_*)y, ldy, B, Li, C, stride));
    OD_CHECK_LAUNCH();
    return 0;
}

extern "C" int od_unet_up_varlen(int dtype, const void* x, int ldx, const float* w, const float* bias, void* y, int ldy, const int* lens,
                                 int B, int Li, int C, int stride, void* stream) {
    if (!lanes_ok(C) || ldx % 8 || ldy % 8) return OD_ERR_ALIGN;
    if (stride < 1 || stride > 8) return OD_ERR_UNSUPPORTED;
    if (!lens) return OD_ERR_ARG;
    const long M = (long)B * Li * stride;
    DISPATCH_T(dtype, OD_LAUNCH((unet_up_kernel<T_, true>), dim3(row_grid(M, C)), dim3(256), 0, (hipStream_t)stream, (const T_*)x, ldx,
                                w, bias, (T_*)y, ldy, B, Li, C, stride, lens));
    OD_CHECK_LAUNCH();
    return 0;
}

extern "C" int od_chart_head(int dtype, const void* x, int ldx, const float* W, const float* bias, float* out, int B, int L, int C,
                             int N, int n_sigmoid, int rms, float eps, void* stream) {
    if (!lanes_ok(C) || ldx % 8) return OD_ERR_ALIGN;
    if (N < 1 || N > 16) return OD_ERR_UNSUPPORTED;
    const long M = (long)B * L;
    DISPATCH_T(dtype, OD_LAUNCH((chart_head_kernel<T_, 16>), dim3(row_grid(M, C)), dim3(256), 0, (hipStream_t)stream, (const T_*)x,
                                ldx, W, bias, out, M, L, C, N, n_sigmoid, rms, eps));
    OD_CHECK_LAUNCH();
    return 0;
}

extern "C" int od_chart_head_varlen(int dtype, const void* x, int ldx, const float* W, const float* bias, float* out, const int* lens,
                                    int B, int L, int C, int N, int n_sigmoid, int rms, float eps, void* stream) {
    if (!lanes_ok(C) || ldx % 8) return OD_ERR_ALIGN;
    if (N < 1 || N > 16) return OD_ERR_UNSUPPORTED;
    if (!lens) return OD_ERR_ARG;
    const long M = (long)B * L;
    DISPATCH_T(dtype, OD_LAUNCH((chart_head_kernel<T_, 16, true>), dim3(row_grid(M, C)), dim3(256), 0, (hipStream_t)stream,
                                (const T_*)x, ldx, W, bias, out, M, L, C, N, n_sigmoid, rms, eps, lens));
    OD_CHECK_LAUNCH();
    return 0;
}

extern "C" int od_attn_pool(int dtype, const void* scores, int lds, const void* values, int ldv, float* out, int B, int L, int Hh,
                            int hd, void* stream) {
    if (hd < 1 || hd > 256 || Hh < 1 || L < 1) return OD_ERR_UNSUPPORTED;
    DISPATCH_T(dtype, OD_LAUNCH((attn_pool_kernel<T_>), dim3(Hh, B), dim3(256), 0, (hipStream_t)stream, (const T_*)scores, lds,
                                (const T_*)values, ldv, out, L, Hh, hd));
    OD_CHECK_LAUNCH();
    return 0;
}

extern "C" int od_attn_pool_varlen(int dtype, const void* scores, int lds, const void* values, int ldv, float* out, const int* lens, int B,
                                   int L, int Hh, int hd, void* stream) {
    if (hd < 1 || hd > 256 || Hh < 1 || L < 1) return OD_ERR_UNSUPPORTED;
    if (!lens) return OD_ERR_ARG;
    DISPATCH_T(dtype, OD_LAUNCH((attn_pool_kernel<T_, true>), dim3(Hh, B), dim3(256), 0, (hipStream_t)stream, (const T_*)scores, lds,
                                (const T_*)values, ldv, out, L, Hh, hd, lens));
    OD_CHECK_LAUNCH();
    return 0;
}

// ================================================================================================================================
// Backward (training) kernels: autograd of the row kernels above.  Same lane layout (G = C/8 lanes own a frame, 16-byte accesses,
// fp32 arithmetic, inv_rms recomputed from the row that is read anyway).  A block walks BW_NIT passes of 256/G frames; the sums over
// frames (gamma, FiLM rows, conv taps, head weights) stay in registers across the passes, meet across the block's frame slots in LDS in
// slot order, and leave as ONE row of column partials per block in the caller's workspace.  partial_sum_kernel then adds the rows of a
// destination in block order: no atomics anywhere, the same bits on every launch.
// ================================================================================================================================
namespace {

constexpr int BW_NIT = 4;        // passes of 256/G frames per block
constexpr int BW_KS = 9;         // widest resample conv: stride 8 -> 1 + 2*(8/2) taps

inline int bw_frames(int C) { return 256 / (C >> 3) * BW_NIT; }
inline long bw_blocks(long n, int C) { const int f = bw_frames(C); return (n + f - 1) / f; }

// acc[e] of every lane (frame slot = threadIdx.x / G, channels c..c+7) summed over the block's frame slots, in slot order -> dst[c + e].
// s_red holds 256 * 8 floats; all 256 threads call it.
__device__ __forceinline__ void block_colsum(const float (&acc)[8], float* s_red, int G, int C, int c, float* __restrict__ dst) {
    const int slot = threadIdx.x / G, nslot = 256 / G;
#pragma unroll
    for (int e = 0; e < 8; e++) s_red[slot * C + c + e] = acc[e];
    __syncthreads();
    for (int t = threadIdx.x; t < C; t += 256) {
        float s = 0.f;
        for (int j = 0; j < nslot; j++) s += s_red[j * C + t];
        dst[t] = s;
    }
    __syncthreads();
}

// out[g * ldo + (col % inner) * sa + (col / inner) * sb] += scale * sum_{j < nb} ws[(g * nb + j) * ncols + col0 + col],  col < n.
// 16 columns x 16 segments per block: a segment adds its contiguous share of the nb rows in order, the 16 segment sums meet in order.
__global__ __launch_bounds__(256) void partial_sum_kernel(const float* __restrict__ ws, int nb, int ncols, int col0, float* __restrict__ out,
                                                          long ldo, int n, int inner, int sa, int sb, float scale) {
    __shared__ float s_seg[16][17];
    const int tc = threadIdx.x & 15, seg = threadIdx.x >> 4;
    const int col = blockIdx.x * 16 + tc, g = blockIdx.y;
    const int per = (nb + 15) / 16;
    const int j0 = seg * per, j1 = j0 + per < nb ? j0 + per : nb;
    float s = 0.f;
    if (col < n)
        for (int j = j0; j < j1; j++) s += ws[((size_t)g * nb + j) * ncols + col0 + col];
    s_seg[seg][tc] = s;
    __syncthreads();
    if (seg == 0 && col < n) {
        float t = 0.f;
#pragma unroll
        for (int k = 0; k < 16; k++) t += s_seg[k][tc];
        out[(size_t)g * ldo + (size_t)(col % inner) * sa + (size_t)(col / inner) * sb] += scale * t;
    }
}

inline void launch_partial_sum(hipStream_t st, const float* ws, int groups, int nb, int ncols, int col0, float* out, long ldo, int n,
                               int inner, int sa, int sb, float scale) {
    OD_LAUNCH(partial_sum_kernel, dim3((n + 15) / 16, groups), dim3(256), 0, st, ws, nb, ncols, col0, out, ldo, n, inner, sa, sb, scale);
}

// frame slot, channel and the block's first frame, for the kernels whose blocks stay inside one batch row (grid: blocks per row x B)
#define OD_BWD_BLOCK_OF_LANE()                                                  \
    const int G = C >> 3, rpp = 256 / G;                                        \
    const int c = (threadIdx.x % G) * 8;                                        \
    const int l0 = blockIdx.x * rpp * BW_NIT + threadIdx.x / G

// y = act(u), u = x^ gamma (1 + scale[b]) + shift[b], x^ = x inv:   du = dy act'(u);  dshift[b] += du;  dscale[b] += du x^ gamma;
// dgamma += du (1 + scale) x^;  with g = du gamma (1 + scale):  dx (+)= inv (g - x^ mean_c(g x^)).        partial row: [dgamma | dscale | dshift]
template <class T>
__global__ __launch_bounds__(256) void rms_affine_film_bwd_kernel(const T* __restrict__ x, int ldx, const float* __restrict__ gamma,
                                                                  const float* __restrict__ ssg, const T* __restrict__ dy, int lddy,
                                                                  T* __restrict__ dx, int lddx, int accumulate, float* __restrict__ ws,
                                                                  int L, int C, float eps, int act) {
    __shared__ float s_red[2048];
    OD_BWD_BLOCK_OF_LANE();
    const int b = blockIdx.y;
    float g[8], sc[8], sh[8];
    od_ld8(gamma + c, g);
#pragma unroll
    for (int e = 0; e < 8; e++) { sc[e] = 1.f; sh[e] = 0.f; }
    if (ssg) {
        float s[8];
        od_ld8(ssg + (size_t)b * 3 * C + c, s);
        od_ld8(ssg + (size_t)b * 3 * C + C + c, sh);
#pragma unroll
        for (int e = 0; e < 8; e++) sc[e] = 1.f + s[e];
    }
    float a_g[8] = {0, 0, 0, 0, 0, 0, 0, 0}, a_s[8] = {0, 0, 0, 0, 0, 0, 0, 0}, a_h[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    for (int it = 0; it < BW_NIT; it++) {
        const int l = l0 + it * rpp;
        const bool live = l < L;
        const long m = (long)b * L + (live ? l : L - 1);      // dead lanes shadow the last frame so shuffles stay convergent
        float v[8], d[8], o[8];
        od_ld8(x + m * ldx + c, v);
        od_ld8(dy + m * lddy + c, d);
        const float inv = rsqrtf(group_sum(sumsq8(v), G) / (float)C + eps);
        float dot = 0.f;
#pragma unroll
        for (int e = 0; e < 8; e++) {
            v[e] *= inv;                                       // x^
            if (act == OD_ACT_SILU) d[e] *= od_silu_grad(v[e] * g[e] * sc[e] + sh[e]);
            if (live) { a_h[e] += d[e]; a_s[e] += d[e] * v[e] * g[e]; a_g[e] += d[e] * sc[e] * v[e]; }
            d[e] *= g[e] * sc[e];
            dot += d[e] * v[e];
        }
        dot = group_sum(dot, G) / (float)C;
#pragma unroll
        for (int e = 0; e < 8; e++) o[e] = inv * (d[e] - v[e] * dot);
        if (live) {
            if (accumulate) {
                float old[8];
                od_ld8(dx + m * lddx + c, old);
#pragma unroll
                for (int e = 0; e < 8; e++) o[e] += old[e];
            }
            od_st8(dx + m * lddx + c, o);
        }
    }
    float* row = ws + ((size_t)b * gridDim.x + blockIdx.x) * 3 * C;
    block_colsum(a_g, s_red, G, C, c, row);
    if (ssg) {
        block_colsum(a_s, s_red, G, C, c, row + C);
        block_colsum(a_h, s_red, G, C, c, row + 2 * C);
    }
}

// xo = x + h^ gamma (1 + gate[b]), h^ = h inv:   dgamma += dxo (1 + gate) h^;  dgate[b] += dxo gamma h^;
// with g = dxo gamma (1 + gate):  dh = inv (g - h^ mean_c(g h^)).                                          partial row: [dgamma | dgate]
template <class T>
__global__ __launch_bounds__(256) void rms_affine_gate_res_bwd_kernel(const T* __restrict__ h, int ldh, const float* __restrict__ gamma,
                                                                      const float* __restrict__ ssg, const T* __restrict__ dxo, int lddxo,
                                                                      T* __restrict__ dh, int lddh, float* __restrict__ ws, int L, int C,
                                                                      float eps) {
    __shared__ float s_red[2048];
    OD_BWD_BLOCK_OF_LANE();
    const int b = blockIdx.y;
    float g[8], gt[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    od_ld8(gamma + c, g);
    if (ssg) od_ld8(ssg + (size_t)b * 3 * C + 2 * C + c, gt);
    float a_g[8] = {0, 0, 0, 0, 0, 0, 0, 0}, a_t[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    for (int it = 0; it < BW_NIT; it++) {
        const int l = l0 + it * rpp;
        const bool live = l < L;
        const long m = (long)b * L + (live ? l : L - 1);
        float v[8], d[8], o[8];
        od_ld8(h + m * ldh + c, v);
        od_ld8(dxo + m * lddxo + c, d);
        const float inv = rsqrtf(group_sum(sumsq8(v), G) / (float)C + eps);
        float dot = 0.f;
#pragma unroll
        for (int e = 0; e < 8; e++) {
            v[e] *= inv;
            if (live) { a_g[e] += d[e] * (1.f + gt[e]) * v[e]; a_t[e] += d[e] * g[e] * v[e]; }
            d[e] *= g[e] * (1.f + gt[e]);
            dot += d[e] * v[e];
        }
        dot = group_sum(dot, G) / (float)C;
#pragma unroll
        for (int e = 0; e < 8; e++) o[e] = inv * (d[e] - v[e] * dot);
        if (live) od_st8(dh + m * lddh + c, o);
    }
    float* row = ws + ((size_t)b * gridDim.x + blockIdx.x) * 2 * C;
    block_colsum(a_g, s_red, G, C, c, row);
    if (ssg) block_colsum(a_t, s_red, G, C, c, row + C);
}

// xo = x + p^ gamma gx, p^ = p inv:   dgx = dxo p^ gamma;  dgamma += dxo p^ gx;  with g = dxo gamma gx:  dp = inv (g - p^ mean_c(g p^)).
// BC (the skip is broadcast): the block's frames are frames of the ONE skip row; a lane walks the batch rows in order, keeps its frame's
// dp in fp32 registers and writes the sum as fp32.                                                         partial row: [dgamma]
template <class T, bool BC>
__global__ __launch_bounds__(256) void mixer_bwd_kernel(const T* __restrict__ p, int ldp, const T* __restrict__ gx, int ldg,
                                                        const float* __restrict__ gamma, const T* __restrict__ dxo, int lddxo,
                                                        void* __restrict__ dp_, int lddp, T* __restrict__ dgx, int lddg,
                                                        float* __restrict__ ws, int B, int L, int C, float eps) {
    __shared__ float s_red[2048];
    OD_BWD_BLOCK_OF_LANE();
    float g[8];
    od_ld8(gamma + c, g);
    float a_g[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    const int b0 = BC ? 0 : blockIdx.y, b1 = BC ? B : blockIdx.y + 1;
    for (int it = 0; it < BW_NIT; it++) {
        const int l = l0 + it * rpp;
        const bool live = l < L;
        const int lr = live ? l : L - 1;
        float v[8], sum[8] = {0, 0, 0, 0, 0, 0, 0, 0};
        float inv = 0.f;
        for (int b = b0; b < b1; b++) {
            const long m = (long)b * L + lr;
            if (!BC || b == b0) {
                od_ld8(p + (BC ? (long)lr : m) * ldp + c, v);
                inv = rsqrtf(group_sum(sumsq8(v), G) / (float)C + eps);
#pragma unroll
                for (int e = 0; e < 8; e++) v[e] *= inv;
            }
            float d[8], q[8], o[8];
            od_ld8(dxo + m * lddxo + c, d);
            od_ld8(gx + m * ldg + c, q);
            float dot = 0.f;
#pragma unroll
            for (int e = 0; e < 8; e++) {
                o[e] = d[e] * v[e] * g[e];
                if (live) a_g[e] += d[e] * v[e] * q[e];
                d[e] *= g[e] * q[e];
                dot += d[e] * v[e];
            }
            if (live) od_st8(dgx + m * lddg + c, o);
            dot = group_sum(dot, G) / (float)C;
#pragma unroll
            for (int e = 0; e < 8; e++) sum[e] += inv * (d[e] - v[e] * dot);
            if (!BC && live) od_st8((T*)dp_ + m * lddp + c, sum);
        }
        if (BC && live) od_st8((float*)dp_ + (long)l * lddp + c, sum);
    }
    float* row = ws + ((size_t)blockIdx.y * gridDim.x + blockIdx.x) * C;
    block_colsum(a_g, s_red, G, C, c, row);
}

// sum of w[c+e][k] over k0 <= k <= k1 (the taps that land on one input frame)
__device__ __forceinline__ void tap_sum(const float* __restrict__ w, int c, int ks, int k0, int k1, float (&ws)[8]) {
#pragma unroll
    for (int e = 0; e < 8; e++) {
        float s = 0.f;
        for (int k = k0; k <= k1; k++) s += w[(c + e) * ks + k];
        ws[e] = s;
    }
}

// od_unet_down, gradient of the input: dx[b][l] = (1/s) sum_lo dy[b][lo] (sum of w[k] over the k + j = l - s lo + r, 0 <= j < s)
template <class T>
__global__ __launch_bounds__(256) void unet_down_bwd_dx_kernel(const float* __restrict__ w, const T* __restrict__ dy, int lddy,
                                                               T* __restrict__ dx, int lddx, int B, int Lo, int C, int s) {
    const int G = C >> 3, r = s / 2, ks = 2 * r + 1, L = Lo * s;
    const long M = (long)B * L;
    const long m = (long)blockIdx.x * (256 / G) + threadIdx.x / G;
    const int c = (threadIdx.x % G) * 8;
    if (m >= M) return;
    const int b = (int)(m / L), l = (int)(m % L);
    const int num = l - (s - 1) - r;
    const int lo_min = num <= 0 ? 0 : (num + s - 1) / s;
    const int lo_max = (l + r) / s < Lo - 1 ? (l + r) / s : Lo - 1;
    float acc[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    for (int lo = lo_min; lo <= lo_max; lo++) {
        const int t = l - s * lo + r;                         // 0 <= t <= s + ks - 2
        const int k0 = t - (s - 1) > 0 ? t - (s - 1) : 0, k1 = t < ks - 1 ? t : ks - 1;
        float d[8], wv[8];
        od_ld8(dy + ((long)b * Lo + lo) * lddy + c, d);
        tap_sum(w, c, ks, k0, k1, wv);
#pragma unroll
        for (int e = 0; e < 8; e++) acc[e] += wv[e] * d[e];
    }
#pragma unroll
    for (int e = 0; e < 8; e++) acc[e] /= (float)s;
    od_st8(dx + m * lddx + c, acc);
}

// od_unet_down, gradients of the taps and the bias, per output frame: db += dy;  dw[k] += dy (1/s) sum_j x[s lo + j + k - r]  (the 1/s is
// applied by the second pass).  UP: od_unet_up instead, per output frame l: dw[k] += dy x[(l + k - r) / s].
// partial row: [dw tap 0 | ... | dw tap ks-1 | db], C columns each
template <class T, bool UP>
__global__ __launch_bounds__(256) void unet_resample_bwd_dw_kernel(const T* __restrict__ x, int ldx, const T* __restrict__ dy, int lddy,
                                                                   float* __restrict__ ws, int B, int Ly, int C, int s) {
    __shared__ float s_red[2048];
    const int G = C >> 3, rpp = 256 / G, r = s / 2, ks = 2 * r + 1;
    const int c = (threadIdx.x % G) * 8;
    const long M = (long)B * Ly;                              // frames of dy
    const int Lx = UP ? Ly / s : Ly * s;                      // frames of x per batch row
    const int Lu = UP ? Ly : Lx;                              // the conv's own length (it runs at the fine level both ways)
    float a_w[BW_KS][8], a_b[8] = {0, 0, 0, 0, 0, 0, 0, 0};
#pragma unroll
    for (int k = 0; k < BW_KS; k++)
#pragma unroll
        for (int e = 0; e < 8; e++) a_w[k][e] = 0.f;
    for (int it = 0; it < BW_NIT; it++) {
        const long m = ((long)blockIdx.x * BW_NIT + it) * rpp + threadIdx.x / G;
        if (m >= M) continue;
        const int b = (int)(m / Ly), ly = (int)(m % Ly);
        float d[8];
        od_ld8(dy + m * lddy + c, d);
#pragma unroll
        for (int e = 0; e < 8; e++) a_b[e] += d[e];
        if (UP) {
#pragma unroll
            for (int k = 0; k < BW_KS; k++) {
                const int lu = ly + k - r;
                if (k >= ks || lu < 0 || lu >= Lu) continue;
                float v[8];
                od_ld8(x + ((long)b * Lx + lu / s) * ldx + c, v);
#pragma unroll
                for (int e = 0; e < 8; e++) a_w[k][e] += d[e] * v[e];
            }
        } else {
            for (int t = 0; t < s + ks - 1; t++) {
                const int l = s * ly - r + t;
                if (l < 0 || l >= Lu) continue;
                float v[8];
                od_ld8(x + ((long)b * Lx + l) * ldx + c, v);
#pragma unroll
                for (int k = 0; k < BW_KS; k++) {
                    const int j = t - k;
                    if (k < ks && j >= 0 && j < s) {
#pragma unroll
                        for (int e = 0; e < 8; e++) a_w[k][e] += d[e] * v[e];
                    }
                }
            }
        }
    }
    float* row = ws + (size_t)blockIdx.x * (ks + 1) * C;
#pragma unroll
    for (int k = 0; k < BW_KS; k++)
        if (k < ks) block_colsum(a_w[k], s_red, G, C, c, row + (size_t)k * C);
    block_colsum(a_b, s_red, G, C, c, row + (size_t)ks * C);
}

// od_unet_up, gradient of the input: dx[b][li] = sum_l dy[b][l] (sum of w[k] over s li <= l + k - r <= s li + s - 1)
template <class T>
__global__ __launch_bounds__(256) void unet_up_bwd_dx_kernel(const float* __restrict__ w, const T* __restrict__ dy, int lddy,
                                                             T* __restrict__ dx, int lddx, int B, int Li, int C, int s) {
    const int G = C >> 3, r = s / 2, ks = 2 * r + 1, L = Li * s;
    const long M = (long)B * Li;
    const long m = (long)blockIdx.x * (256 / G) + threadIdx.x / G;
    const int c = (threadIdx.x % G) * 8;
    if (m >= M) return;
    const int b = (int)(m / Li), li = (int)(m % Li);
    float acc[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    for (int l = s * li - r; l <= s * li + s - 1 + r; l++) {
        if (l < 0 || l >= L) continue;
        const int k0 = s * li - l + r > 0 ? s * li - l + r : 0;
        const int k1 = s * li + s - 1 - l + r < ks - 1 ? s * li + s - 1 - l + r : ks - 1;
        float d[8], wv[8];
        od_ld8(dy + ((long)b * L + l) * lddy + c, d);
        tap_sum(w, c, ks, k0, k1, wv);
#pragma unroll
        for (int e = 0; e < 8; e++) acc[e] += wv[e] * d[e];
    }
    od_st8(dx + m * lddx + c, acc);
}

// od_chart_head (n_sigmoid = 0): y_n = bias_n + W_n . x;  out_n = y_n k, k = rsqrt(mean_n y^2 + eps) when rms, else y_n.
// dy_n = k (dout_n - y^_n mean_n(dout y^)) (rms) or dout_n;  dx = sum_n dy_n W_n;  dW_n += dy_n x;  db_n += dy_n.
// partial row: [dW row 0 | ... | dW row N-1 | db (N)]
template <class T, int NMAX>
__global__ __launch_bounds__(256) void chart_head_bwd_kernel(const T* __restrict__ x, int ldx, const float* __restrict__ W,
                                                             const float* __restrict__ bias, const float* __restrict__ dout,
                                                             T* __restrict__ dx, int lddx, float* __restrict__ ws, long M, int L, int C,
                                                             int N, int rms, float eps) {
    __shared__ float s_red[2048];
    const int G = C >> 3, rpp = 256 / G;
    const int c = (threadIdx.x % G) * 8, slot = threadIdx.x / G;
    float a_w[NMAX][8], a_b[NMAX];
#pragma unroll
    for (int n = 0; n < NMAX; n++) {
        a_b[n] = 0.f;
#pragma unroll
        for (int e = 0; e < 8; e++) a_w[n][e] = 0.f;
    }
    for (int it = 0; it < BW_NIT; it++) {
        const long m = ((long)blockIdx.x * BW_NIT + it) * rpp + slot;
        const bool live = m < M;
        const long mr = live ? m : M - 1;
        const int b = (int)(mr / L), l = (int)(mr % L);
        float v[8], dyv[NMAX], ss = 0.f, dd = 0.f;
        od_ld8(x + mr * ldx + c, v);
#pragma unroll
        for (int n = 0; n < NMAX; n++) {
            dyv[n] = 0.f;
            if (n >= N) continue;
            dyv[n] = dout[((size_t)b * N + n) * L + l];
            if (rms) {
                float wv[8], s = 0.f;
                od_ld8(W + (size_t)n * C + c, wv);
#pragma unroll
                for (int e = 0; e < 8; e++) s += wv[e] * v[e];
                s = group_sum(s, G) + bias[n];
                ss += s * s; dd += dyv[n] * s;                 // y_n is recomputed below rather than held in NMAX more registers
            }
        }
        float o[8] = {0, 0, 0, 0, 0, 0, 0, 0};
        const float k = rms ? rsqrtf(ss / (float)N + eps) : 1.f;
        const float mean = dd * k / (float)N;                 // mean_n(dout y^)
#pragma unroll
        for (int n = 0; n < NMAX; n++) {
            if (n >= N) continue;
            float wv[8];
            od_ld8(W + (size_t)n * C + c, wv);
            float g = dyv[n];
            if (rms) {
                float s = 0.f;
#pragma unroll
                for (int e = 0; e < 8; e++) s += wv[e] * v[e];
                s = group_sum(s, G) + bias[n];
                g = k * (g - s * k * mean);
            }
            if (live) {
                a_b[n] += g;
#pragma unroll
                for (int e = 0; e < 8; e++) a_w[n][e] += g * v[e];
            }
#pragma unroll
            for (int e = 0; e < 8; e++) o[e] += g * wv[e];
        }
        if (live) od_st8(dx + m * lddx + c, o);
    }
    float* row = ws + (size_t)blockIdx.x * N * (C + 1);
#pragma unroll
    for (int n = 0; n < NMAX; n++)
        if (n < N) block_colsum(a_w[n], s_red, G, C, c, row + (size_t)n * C);
    // db: every lane of a frame holds the same dy_n; the frame's first lane hands it over, `per` outputs a round so that the rpp slots
    // fit s_red (C = 8: 256 slots x 8, two rounds; wider C: one round of NMAX)
    const int per = 2048 / rpp < NMAX ? 2048 / rpp : NMAX;
    for (int n0 = 0; n0 < N; n0 += per) {
#pragma unroll
        for (int n = 0; n < NMAX; n++)
            if (c == 0 && n >= n0 && n < n0 + per) s_red[slot * per + n - n0] = a_b[n];
        __syncthreads();
        const int n = n0 + (int)threadIdx.x;
        if ((int)threadIdx.x < per && n < N) {
            float s = 0.f;
            for (int j = 0; j < rpp; j++) s += s_red[j * per + threadIdx.x];
            row[(size_t)N * C + n] = s;
        }
        __syncthreads();
    }
}

// AttnPool backward, one block per (b, h); G2 = hd/8 lanes own a frame's head slice.  With p = softmax_l(scores), dot_l = dout . v_l:
// dv_l = p_l dout;  dscore_l = p_l (dot_l - sum_l' p_l' dot_l').  Block sums (max, denominator, sum p dot) go through LDS trees in a fixed order.
__device__ __forceinline__ float block_tree(float v, float* red, bool is_max) {
    const int t = threadIdx.x;
    red[t] = v;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if (t < s) red[t] = is_max ? fmaxf(red[t], red[t + s]) : red[t] + red[t + s];
        __syncthreads();
    }
    const float out = red[0];
    __syncthreads();
    return out;
}
template <class T>
__global__ __launch_bounds__(256) void attn_pool_bwd_kernel(const T* __restrict__ scores, int lds_, const T* __restrict__ values, int ldv,
                                                            const float* __restrict__ dout, T* __restrict__ dscores, int ldds,
                                                            T* __restrict__ dvalues, int lddv, int L, int Hh, int hd) {
    __shared__ float red[256];
    const int b = blockIdx.y, h = blockIdx.x, t = threadIdx.x;
    const int G2 = hd >> 3, fpp = 256 / G2, slot = t / G2, c = (t % G2) * 8;
    const T* sb = scores + (size_t)b * L * lds_ + h;
    float mx = -3.0e38f;
    for (int l = t; l < L; l += 256) mx = fmaxf(mx, od_t<T>::ld(sb + (size_t)l * lds_));
    mx = block_tree(mx, red, true);
    float go[8];
    od_ld8(dout + ((size_t)b * Hh + h) * hd + c, go);
    float den = 0.f, pd = 0.f;
    for (int l0 = 0; l0 < L; l0 += fpp) {
        const int l = l0 + slot;
        const bool live = l < L;
        const int lr = live ? l : L - 1;
        float v[8], dot = 0.f;
        od_ld8(values + ((size_t)b * L + lr) * ldv + h * hd + c, v);
#pragma unroll
        for (int e = 0; e < 8; e++) dot += go[e] * v[e];
        dot = group_sum(dot, G2);
        const float ex = __expf(od_t<T>::ld(sb + (size_t)lr * lds_) - mx);
        if (live && c == 0) { den += ex; pd += ex * dot; }
    }
    den = block_tree(den, red, false);
    pd = block_tree(pd, red, false) / den;                   // sum_l p_l dot_l
    for (int l0 = 0; l0 < L; l0 += fpp) {
        const int l = l0 + slot;
        const bool live = l < L;
        const int lr = live ? l : L - 1;
        float v[8], o[8], dot = 0.f;
        od_ld8(values + ((size_t)b * L + lr) * ldv + h * hd + c, v);
#pragma unroll
        for (int e = 0; e < 8; e++) dot += go[e] * v[e];
        dot = group_sum(dot, G2);
        const float pl = __expf(od_t<T>::ld(sb + (size_t)lr * lds_) - mx) / den;
#pragma unroll
        for (int e = 0; e < 8; e++) o[e] = pl * go[e];
        if (live) {
            od_st8(dvalues + ((size_t)b * L + l) * lddv + h * hd + c, o);
            if (c == 0) od_t<T>::st(dscores + ((size_t)b * L + l) * ldds + h, pl * (dot - pd));
        }
    }
}

// dxt[b][e][l] = sum_c W[c][e] dx[(b,l)][c]
template <class T>
__global__ __launch_bounds__(256) void proj_in_bwd_input_kernel(const T* __restrict__ dx, int ldx, const float* __restrict__ W,
                                                                float* __restrict__ dxt, long M, int L, int C, int E) {
    OD_ROW_OF_LANE();
    float d[8], acc[8];
    od_ld8(dx + mr * ldx + c, d);
#pragma unroll
    for (int e = 0; e < 8; e++) {
        float s = 0.f;
        if (e < E) {
#pragma unroll
            for (int i = 0; i < 8; i++) s += W[(size_t)(c + i) * E + e] * d[i];
        }
        acc[e] = group_sum(s, G);
    }
    const int b = (int)(mr / L), l = (int)(mr % L);
#pragma unroll
    for (int e = 0; e < 8; e++)
        if (e < E && live && c == 0) dxt[((size_t)b * E + e) * L + l] = acc[e];
}

// SpecFeatures front end, backward (parameters only: the spectrogram takes no gradient).  One block owns SFB_TL frames of one batch row,
// recomputes stage 1 with a 2-frame halo and stage 2 with a 1-frame halo (the gradient of an owned stage-1 frame comes from the stage-2
// frames either side), and keeps in LDS: the spectrogram tile, h1, the gradient at conv2's output (dacc2) and one more plane that first
// holds the g2 terms and then the gradient at conv1's output (dacc1); the g1 terms reuse h1's storage once conv2's weights are done.
// Every parameter's sum over the block's positions is formed by ONE thread walking the positions in order (gather form, no LDS atomics)
// and written straight into the block's partial row: [dw1 192 | db1 8 | dg1 8 | dw2 4608 | db2 32 | dg2 32].
constexpr int SFB_TL = 32;
constexpr int SFB_W1 = SF_C1 * 8 * 3, SFB_W2 = SF_C2 * SF_C1 * 6 * 3;
constexpr int SFB_COLS = SFB_W1 + 2 * SF_C1 + SFB_W2 + 2 * SF_C2;
template <class T>
__global__ __launch_bounds__(256) void spec_conv_bwd_kernel(const float* __restrict__ audio, const float* __restrict__ w1,
                                                            const float* __restrict__ b1, const float* __restrict__ g1,
                                                            const float* __restrict__ w2, const float* __restrict__ b2,
                                                            const float* __restrict__ g2, const T* __restrict__ dout, int ldo,
                                                            float* __restrict__ ws, int L, float eps) {
    __shared__ float s_in[SF_F + 2][SFB_TL + 6];               // freq rows -1..72, frames l0-3 .. l0+TL+2
    __shared__ float s_h1[SF_C1][SF_A1 + 2][SFB_TL + 4];       // freq rows -1..12, frames l0-2 .. l0+TL+1
    __shared__ float s_d2[SF_C2][SF_A2][SFB_TL + 2];           // dacc2, frames l0-1 .. l0+TL
    __shared__ float s_r2[SF_C2 * SF_A2 * SFB_TL];             // g2 terms [c2][a2][t], then dacc1 [cc][a1][t] (the same size)
    float* s_t1 = &s_h1[0][0][0];                              // g1 terms [cc][a1][t], once h1 is dead
    const int b = blockIdx.y, l0 = blockIdx.x * SFB_TL, tid = threadIdx.x;
    const float* ab = audio + (size_t)b * SF_F * L;
    for (int i = tid; i < (SF_F + 2) * (SFB_TL + 6); i += 256) {
        const int f = i / (SFB_TL + 6) - 1, t = i % (SFB_TL + 6), l = l0 - 3 + t;
        s_in[f + 1][t] = (f >= 0 && f < SF_F && l >= 0 && l < L) ? ab[(size_t)f * L + l] : 0.f;
    }
    for (int i = tid; i < SF_C1 * 2 * (SFB_TL + 4); i += 256) {   // zero freq border of h1
        const int cc = i / (2 * (SFB_TL + 4)), rr = (i / (SFB_TL + 4)) % 2, t = i % (SFB_TL + 4);
        s_h1[cc][rr ? SF_A1 + 1 : 0][t] = 0.f;
    }
    __syncthreads();
    // stage 1 forward: h1 = SiLU(rms(conv1) g1), zero outside the sequence (conv2's time padding)
    for (int i = tid; i < SF_A1 * (SFB_TL + 4); i += 256) {
        const int a = i / (SFB_TL + 4), t = i % (SFB_TL + 4), l = l0 - 2 + t;
        float acc[SF_C1];
#pragma unroll
        for (int cc = 0; cc < SF_C1; cc++) acc[cc] = b1[cc];
        for (int fi = 0; fi < 8; fi++)
#pragma unroll
            for (int j = 0; j < 3; j++) {
                const float v = s_in[6 * a + fi][t + j];
#pragma unroll
                for (int cc = 0; cc < SF_C1; cc++) acc[cc] += w1[(cc * 8 + fi) * 3 + j] * v;
            }
        float ss = 0.f;
#pragma unroll
        for (int cc = 0; cc < SF_C1; cc++) ss += acc[cc] * acc[cc];
        const float inv = rsqrtf(ss / (float)SF_C1 + eps);
        const bool inside = l >= 0 && l < L;
#pragma unroll
        for (int cc = 0; cc < SF_C1; cc++) s_h1[cc][a + 1][t] = inside ? od_silu(acc[cc] * inv * g1[cc]) : 0.f;
    }
    __syncthreads();
    // stage 2 forward and its backward down to conv2's output: dacc2 (0 outside the sequence) and the g2 terms of the owned frames
    for (int i = tid; i < SF_A2 * (SFB_TL + 2); i += 256) {
        const int a = i / (SFB_TL + 2), t = i % (SFB_TL + 2), l = l0 - 1 + t;
        const bool inside = l >= 0 && l < L, owned = inside && t >= 1 && t <= SFB_TL;
        float acc[SF_C2];
#pragma unroll
        for (int c2 = 0; c2 < SF_C2; c2++) acc[c2] = b2[c2];
        if (inside) {
#pragma unroll 1
            for (int cc = 0; cc < SF_C1; cc++)
#pragma unroll 1
                for (int fi = 0; fi < 6; fi++)
#pragma unroll
                    for (int j = 0; j < 3; j++) {
                        const float v = s_h1[cc][4 * a + fi][t + j];
#pragma unroll
                        for (int c2 = 0; c2 < SF_C2; c2++) acc[c2] += w2[((c2 * SF_C1 + cc) * 6 + fi) * 3 + j] * v;
                    }
        }
        float ss = 0.f;
#pragma unroll
        for (int c2 = 0; c2 < SF_C2; c2++) ss += acc[c2] * acc[c2];
        const float inv = rsqrtf(ss / (float)SF_C2 + eps);
        const T* drow = dout + ((size_t)b * L + (inside ? l : 0)) * ldo;
        float dot = 0.f;
#pragma unroll
        for (int c2 = 0; c2 < SF_C2; c2++) {
            const float xh = acc[c2] * inv;
            const float du = inside ? od_t<T>::ld(drow + c2 * SF_A2 + a) * od_silu_grad(xh * g2[c2]) : 0.f;
            if (owned) s_r2[(c2 * SF_A2 + a) * SFB_TL + t - 1] = du * xh;
            else if (t >= 1 && t <= SFB_TL) s_r2[(c2 * SF_A2 + a) * SFB_TL + t - 1] = 0.f;
            acc[c2] = xh;
            dot += du * g2[c2] * xh;
            s_d2[c2][a][t] = du * g2[c2];                      // d x^, finished below
        }
        dot /= (float)SF_C2;
#pragma unroll
        for (int c2 = 0; c2 < SF_C2; c2++) s_d2[c2][a][t] = inv * (s_d2[c2][a][t] - acc[c2] * dot);
    }
    __syncthreads();
    float* row = ws + ((size_t)b * gridDim.x + blockIdx.x) * SFB_COLS;
    // conv2's weights: dw2[c2][cc][fi][j] = sum over the owned (a2, t) of dacc2[c2][a2][t] h1[cc][4 a2 + fi][t + j]
    for (int i = tid; i < SFB_W2; i += 256) {
        const int j = i % 3, fi = (i / 3) % 6, cc = (i / 18) % SF_C1, c2 = i / (18 * SF_C1);
        float s = 0.f;
        for (int a = 0; a < SF_A2; a++)
            for (int t = 1; t <= SFB_TL; t++) s += s_d2[c2][a][t] * s_h1[cc][4 * a + fi][t + j];
        row[SFB_W1 + 2 * SF_C1 + i] = s;
    }
    if (tid < 2 * SF_C2) {
        const int c2 = tid % SF_C2;
        float s = 0.f;
        for (int a = 0; a < SF_A2; a++)
            for (int t = 0; t < SFB_TL; t++) s += tid < SF_C2 ? s_d2[c2][a][t + 1] : s_r2[(c2 * SF_A2 + a) * SFB_TL + t];
        row[SFB_W1 + 2 * SF_C1 + SFB_W2 + tid] = s;            // db2 then dg2
    }
    __syncthreads();
    // gradient of the owned h1 positions (gathered from dacc2), through SiLU and the norm to conv1's output
    for (int i = tid; i < SF_A1 * SFB_TL; i += 256) {
        const int a1 = i / SFB_TL, t = i % SFB_TL, l = l0 + t;   // h1 row a1 + 1, column t + 2
        float dh[SF_C1], acc[SF_C1];
#pragma unroll
        for (int cc = 0; cc < SF_C1; cc++) { dh[cc] = 0.f; acc[cc] = b1[cc]; }
        for (int a2 = 0; a2 < SF_A2; a2++) {
            const int fi = a1 + 1 - 4 * a2;
            if (fi < 0 || fi >= 6) continue;
#pragma unroll
            for (int j = 0; j < 3; j++)
#pragma unroll 4
                for (int c2 = 0; c2 < SF_C2; c2++) {
                    const float d = s_d2[c2][a2][t - j + 2];
#pragma unroll
                    for (int cc = 0; cc < SF_C1; cc++) dh[cc] += w2[((c2 * SF_C1 + cc) * 6 + fi) * 3 + j] * d;
                }
        }
        for (int fi = 0; fi < 8; fi++)
#pragma unroll
            for (int j = 0; j < 3; j++) {
                const float v = s_in[6 * a1 + fi][t + 2 + j];
#pragma unroll
                for (int cc = 0; cc < SF_C1; cc++) acc[cc] += w1[(cc * 8 + fi) * 3 + j] * v;
            }
        float ss = 0.f, dot = 0.f;
#pragma unroll
        for (int cc = 0; cc < SF_C1; cc++) ss += acc[cc] * acc[cc];
        const float inv = rsqrtf(ss / (float)SF_C1 + eps);
        const bool inside = l < L;
#pragma unroll
        for (int cc = 0; cc < SF_C1; cc++) {
            const float xh = acc[cc] * inv;
            const float du = inside ? dh[cc] * od_silu_grad(xh * g1[cc]) : 0.f;
            acc[cc] = xh;
            dh[cc] = du * g1[cc];
            dot += dh[cc] * xh;
            s_t1[(cc * SF_A1 + a1) * SFB_TL + t] = du * xh;
        }
        dot /= (float)SF_C1;
#pragma unroll
        for (int cc = 0; cc < SF_C1; cc++) s_r2[(cc * SF_A1 + a1) * SFB_TL + t] = inv * (dh[cc] - acc[cc] * dot);
    }
    __syncthreads();
    // conv1's weights: dw1[cc][fi][j] = sum over the owned (a1, t) of dacc1[cc][a1][t] in[6 a1 + fi][t + 2 + j]
    if (tid < SFB_W1) {
        const int j = tid % 3, fi = (tid / 3) % 8, cc = tid / 24;
        float s = 0.f;
        for (int a = 0; a < SF_A1; a++)
            for (int t = 0; t < SFB_TL; t++) s += s_r2[(cc * SF_A1 + a) * SFB_TL + t] * s_in[6 * a + fi][t + 2 + j];
        row[tid] = s;
    } else if (tid < SFB_W1 + 2 * SF_C1) {
        const int k = tid - SFB_W1, cc = k % SF_C1;
        const float* src = k < SF_C1 ? s_r2 : s_t1;
        float s = 0.f;
        for (int n = 0; n < SF_A1 * SFB_TL; n++) s += src[cc * SF_A1 * SFB_TL + n];
        row[tid] = s;                                          // db1 then dg1
    }
}

// y[i] += x[i]: where two branches' gradients of one activation meet (the chart encoder's h feeds the style head and the temporal layer)
template <class T>
__global__ __launch_bounds__(256) void add_rows_kernel(const T* __restrict__ x, T* __restrict__ y, long n8) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n8) return;
    float a[8], b[8];
    od_ld8(x + i * 8, a);
    od_ld8(y + i * 8, b);
#pragma unroll
    for (int e = 0; e < 8; e++) b[e] += a[e];
    od_st8(y + i * 8, b);
}

}  // namespace

extern "C" int od_latent_bwd_block_frames(int C) { return lanes_ok(C) ? bw_frames(C) : 0; }

extern "C" int od_rmsnorm_affine_film_bwd(int dtype, const void* x, int ldx, const float* gamma, const float* ssg, const void* dy, int lddy,
                                          void* dx, int lddx, int accumulate_dx, float* dgamma, float* dssg, float* ws, long ws_floats, int B,
                                          int L, int C, float eps, int act, void* stream) {
    if (!lanes_ok(C) || ldx % 8 || lddy % 8 || lddx % 8) return OD_ERR_ALIGN;
    if (B <= 0 || L <= 0 || !dx || !dgamma || !ws || (ssg && !dssg)) return OD_ERR_ARG;
    const int nbl = (int)bw_blocks(L, C);
    if (ws_floats < (long)B * nbl * 3 * C) return OD_ERR_ARG;
    DISPATCH_T(dtype, OD_LAUNCH((rms_affine_film_bwd_kernel<T_>), dim3(nbl, B), dim3(256), 0, (hipStream_t)stream, (const T_*)x, ldx, gamma,
                                ssg, (const T_*)dy, lddy, (T_*)dx, lddx, accumulate_dx, ws, L, C, eps, act));
    launch_partial_sum((hipStream_t)stream, ws, 1, B * nbl, 3 * C, 0, dgamma, 0, C, C, 1, 0, 1.f);
    if (ssg) launch_partial_sum((hipStream_t)stream, ws, B, nbl, 3 * C, C, dssg, 3 * C, 2 * C, 2 * C, 1, 0, 1.f);
    OD_CHECK_LAUNCH();
    return 0;
}

extern "C" int od_rmsnorm_affine_gate_residual_bwd(int dtype, const void* h, int ldh, const float* gamma, const float* ssg, const void* dxo,
                                                   int lddxo, void* dh, int lddh, float* dgamma, float* dssg, float* ws, long ws_floats,
                                                   int B, int L, int C, float eps, void* stream) {
    if (!lanes_ok(C) || ldh % 8 || lddxo % 8 || lddh % 8) return OD_ERR_ALIGN;
    if (B <= 0 || L <= 0 || !dh || !dgamma || !ws || (ssg && !dssg)) return OD_ERR_ARG;
    const int nbl = (int)bw_blocks(L, C);
    if (ws_floats < (long)B * nbl * 2 * C) return OD_ERR_ARG;
    DISPATCH_T(dtype, OD_LAUNCH((rms_affine_gate_res_bwd_kernel<T_>), dim3(nbl, B), dim3(256), 0, (hipStream_t)stream, (const T_*)h, ldh,
                                gamma, ssg, (const T_*)dxo, lddxo, (T_*)dh, lddh, ws, L, C, eps));
    launch_partial_sum((hipStream_t)stream, ws, 1, B * nbl, 2 * C, 0, dgamma, 0, C, C, 1, 0, 1.f);
    if (ssg) launch_partial_sum((hipStream_t)stream, ws, B, nbl, 2 * C, C, dssg + 2 * C, 3 * C, C, C, 1, 0, 1.f);
    OD_CHECK_LAUNCH();
    return 0;
}

extern "C" int od_unet_mixer_bwd(int dtype, const void* p, int ldp, int p_bcast, const void* gx, int ldg, const float* gamma,
                                 const void* dxo, int lddxo, void* dp, int lddp, void* dgx, int lddg, float* dgamma, float* ws,
                                 long ws_floats, int B, int L, int C, float eps, void* stream) {
    if (!lanes_ok(C) || ldp % 8 || ldg % 8 || lddxo % 8 || lddp % 8 || lddg % 8) return OD_ERR_ALIGN;
    if (B <= 0 || L <= 0 || !dp || !dgx || !dgamma || !ws) return OD_ERR_ARG;
    const int nbl = (int)bw_blocks(L, C), rows = p_bcast ? nbl : B * nbl;
    if (ws_floats < (long)rows * C) return OD_ERR_ARG;
    if (p_bcast)
        DISPATCH_T(dtype, OD_LAUNCH((mixer_bwd_kernel<T_, true>), dim3(nbl, 1), dim3(256), 0, (hipStream_t)stream, (const T_*)p, ldp,
                                    (const T_*)gx, ldg, gamma, (const T_*)dxo, lddxo, dp, lddp, (T_*)dgx, lddg, ws, B, L, C, eps));
    else
        DISPATCH_T(dtype, OD_LAUNCH((mixer_bwd_kernel<T_, false>), dim3(nbl, B), dim3(256), 0, (hipStream_t)stream, (const T_*)p, ldp,
                                    (const T_*)gx, ldg, gamma, (const T_*)dxo, lddxo, dp, lddp, (T_*)dgx, lddg, ws, B, L, C, eps));
    launch_partial_sum((hipStream_t)stream, ws, 1, rows, C, 0, dgamma, 0, C, C, 1, 0, 1.f);
    OD_CHECK_LAUNCH();
    return 0;
}

extern "C" int od_unet_down_bwd(int dtype, const void* x, int ldx, const float* w, const void* dy, int lddy, void* dx, int lddx, float* dw,
                                float* db, float* ws, long ws_floats, int B, int Lo, int C, int stride, void* stream) {
    if (!lanes_ok(C) || ldx % 8 || lddy % 8 || lddx % 8) return OD_ERR_ALIGN;
    if (stride < 1 || stride > 8) return OD_ERR_UNSUPPORTED;
    if (B <= 0 || Lo <= 0 || !dx || !dw || !db || !ws) return OD_ERR_ARG;
    const int ks = 2 * (stride / 2) + 1;
    const long My = (long)B * Lo, Mx = My * stride;
    const int nb = (int)bw_blocks(My, C);
    if (ws_floats < (long)nb * (ks + 1) * C) return OD_ERR_ARG;
    DISPATCH_T(dtype, OD_LAUNCH((unet_down_bwd_dx_kernel<T_>), dim3(row_grid(Mx, C)), dim3(256), 0, (hipStream_t)stream, w, (const T_*)dy,
                                lddy, (T_*)dx, lddx, B, Lo, C, stride));
    DISPATCH_T(dtype, OD_LAUNCH((unet_resample_bwd_dw_kernel<T_, false>), dim3(nb), dim3(256), 0, (hipStream_t)stream, (const T_*)x, ldx,
                                (const T_*)dy, lddy, ws, B, Lo, C, stride));
    launch_partial_sum((hipStream_t)stream, ws, 1, nb, (ks + 1) * C, 0, dw, 0, ks * C, C, ks, 1, 1.f / (float)stride);
    launch_partial_sum((hipStream_t)stream, ws, 1, nb, (ks + 1) * C, ks * C, db, 0, C, C, 1, 0, 1.f);
    OD_CHECK_LAUNCH();
    return 0;
}

extern "C" int od_unet_up_bwd(int dtype, const void* x, int ldx, const float* w, const void* dy, int lddy, void* dx, int lddx, float* dw,
                              float* db, float* ws, long ws_floats, int B, int Li, int C, int stride, void* stream) {
    if (!lanes_ok(C) || ldx % 8 || lddy % 8 || lddx % 8) return OD_ERR_ALIGN;
    if (stride < 1 || stride > 8) return OD_ERR_UNSUPPORTED;
    if (B <= 0 || Li <= 0 || !dx || !dw || !db || !ws) return OD_ERR_ARG;
    const int ks = 2 * (stride / 2) + 1;
    const long Mx = (long)B * Li, My = Mx * stride;
    const int nb = (int)bw_blocks(My, C);
    if (ws_floats < (long)nb * (ks + 1) * C) return OD_ERR_ARG;
    DISPATCH_T(dtype, OD_LAUNCH((unet_up_bwd_dx_kernel<T_>), dim3(row_grid(Mx, C)), dim3(256), 0, (hipStream_t)stream, w, (const T_*)dy,
                                lddy, (T_*)dx, lddx, B, Li, C, stride));
    DISPATCH_T(dtype, OD_LAUNCH((unet_resample_bwd_dw_kernel<T_, true>), dim3(nb), dim3(256), 0, (hipStream_t)stream, (const T_*)x, ldx,
                                (const T_*)dy, lddy, ws, B, Li * stride, C, stride));
    launch_partial_sum((hipStream_t)stream, ws, 1, nb, (ks + 1) * C, 0, dw, 0, ks * C, C, ks, 1, 1.f);
    launch_partial_sum((hipStream_t)stream, ws, 1, nb, (ks + 1) * C, ks * C, db, 0, C, C, 1, 0, 1.f);
    OD_CHECK_LAUNCH();
    return 0;
}

extern "C" int od_chart_head_bwd(int dtype, const void* x, int ldx, const float* W, const float* bias, const float* dout, void* dx, int lddx,
                                 float* dW, float* db, float* ws, long ws_floats, int B, int L, int C, int N, int rms, float eps,
                                 void* stream) {
    if (!lanes_ok(C) || ldx % 8 || lddx % 8) return OD_ERR_ALIGN;
    if (N < 1 || N > 16) return OD_ERR_UNSUPPORTED;
    if (B <= 0 || L <= 0 || !dx || !dW || !db || !ws) return OD_ERR_ARG;
    const long M = (long)B * L;
    const int nb = (int)bw_blocks(M, C);
    if (ws_floats < (long)nb * N * (C + 1)) return OD_ERR_ARG;
    DISPATCH_T(dtype, OD_LAUNCH((chart_head_bwd_kernel<T_, 16>), dim3(nb), dim3(256), 0, (hipStream_t)stream, (const T_*)x, ldx, W, bias, dout,
                                (T_*)dx, lddx, ws, M, L, C, N, rms, eps));
    launch_partial_sum((hipStream_t)stream, ws, 1, nb, N * (C + 1), 0, dW, 0, N * C, N * C, 1, 0, 1.f);
    launch_partial_sum((hipStream_t)stream, ws, 1, nb, N * (C + 1), N * C, db, 0, N, N, 1, 0, 1.f);
    OD_CHECK_LAUNCH();
    return 0;
}

extern "C" int od_attn_pool_bwd(int dtype, const void* scores, int lds, const void* values, int ldv, const float* dout, void* dscores,
                                int ldds, void* dvalues, int lddv, int B, int L, int Hh, int hd, void* stream) {
    if (hd < 8 || hd > 256 || (hd & (hd - 1)) || Hh < 1 || L < 1 || B < 1) return OD_ERR_UNSUPPORTED;
    if (ldv % 8 || lddv % 8) return OD_ERR_ALIGN;
    if (!dscores || !dvalues || !dout) return OD_ERR_ARG;
    DISPATCH_T(dtype, OD_LAUNCH((attn_pool_bwd_kernel<T_>), dim3(Hh, B), dim3(256), 0, (hipStream_t)stream, (const T_*)scores, lds,
                                (const T_*)values, ldv, dout, (T_*)dscores, ldds, (T_*)dvalues, lddv, L, Hh, hd));
    OD_CHECK_LAUNCH();
    return 0;
}

extern "C" int od_proj_in_bwd_input(int dtype, const void* dx, int ldx, const float* W, float* dxt, int B, int E, int L, int D,
                                    void* stream) {
    if (E < 1 || E > 8) return OD_ERR_UNSUPPORTED;
    if (!lanes_ok(D) || ldx % 8) return OD_ERR_ALIGN;
    if (B <= 0 || L <= 0 || !dxt) return OD_ERR_ARG;
    const long M = (long)B * L;
    DISPATCH_T(dtype, OD_LAUNCH((proj_in_bwd_input_kernel<T_>), dim3(row_grid(M, D)), dim3(256), 0, (hipStream_t)stream, (const T_*)dx, ldx,
                                W, dxt, M, L, D, E));
    OD_CHECK_LAUNCH();
    return 0;
}

extern "C" int od_spec_features_conv_bwd(int dtype, const float* audio, const float* w1, const float* b1, const float* g1, const float* w2,
                                         const float* b2, const float* g2, const void* dout, int ldo, float* dw1, float* db1, float* dg1,
                                         float* dw2, float* db2, float* dg2, float* ws, long ws_floats, int B, int F, int L, float eps,
                                         void* stream) {
    if (F != SF_F) return OD_ERR_UNSUPPORTED;
    if (B <= 0 || L <= 0 || !dw1 || !db1 || !dg1 || !dw2 || !db2 || !dg2 || !ws) return OD_ERR_ARG;
    const int nbl = (L + SFB_TL - 1) / SFB_TL;
    if (ws_floats < (long)B * nbl * SFB_COLS) return OD_ERR_ARG;
    hipStream_t st = (hipStream_t)stream;
    DISPATCH_T(dtype, OD_LAUNCH((spec_conv_bwd_kernel<T_>), dim3(nbl, B), dim3(256), 0, st, audio, w1, b1, g1, w2, b2, g2, (const T_*)dout,
                                ldo, ws, L, eps));
    const int nb = B * nbl, o2 = SFB_W1 + 2 * SF_C1;
    launch_partial_sum(st, ws, 1, nb, SFB_COLS, 0, dw1, 0, SFB_W1, SFB_W1, 1, 0, 1.f);
    launch_partial_sum(st, ws, 1, nb, SFB_COLS, SFB_W1, db1, 0, SF_C1, SF_C1, 1, 0, 1.f);
    launch_partial_sum(st, ws, 1, nb, SFB_COLS, SFB_W1 + SF_C1, dg1, 0, SF_C1, SF_C1, 1, 0, 1.f);
    launch_partial_sum(st, ws, 1, nb, SFB_COLS, o2, dw2, 0, SFB_W2, SFB_W2, 1, 0, 1.f);
    launch_partial_sum(st, ws, 1, nb, SFB_COLS, o2 + SFB_W2, db2, 0, SF_C2, SF_C2, 1, 0, 1.f);
    launch_partial_sum(st, ws, 1, nb, SFB_COLS, o2 + SFB_W2 + SF_C2, dg2, 0, SF_C2, SF_C2, 1, 0, 1.f);
    OD_CHECK_LAUNCH();
    return 0;
}

extern "C" int od_add_rows(int dtype, const void* x, void* y, long n, void* stream) {
    if (n <= 0 || !x || !y) return OD_ERR_ARG;
    if (n % 8) return OD_ERR_ALIGN;
    DISPATCH_T(dtype, OD_LAUNCH((add_rows_kernel<T_>), dim3((unsigned)((n / 8 + 255) / 256)), dim3(256), 0, (hipStream_t)stream,
                                (const T_*)x, (T_*)y, n / 8));
    OD_CHECK_LAUNCH();
    return 0;
}

// ================================================================================================================================
// Training-step kernels of LatentTrainer (latent/train.py:86-149): the WAE regulariser, the decoder-input perturbation and the
// reconstruction loss with its gradient.  All fp32.  Sums over elements leave a block as one partial row and are added by one block in
// row order (a fixed tree inside a block): no atomics, the same bits on every launch.
// ================================================================================================================================
namespace {

constexpr int LL_T = 256;        // frames of one batch row a block of the loss kernels owns (one per thread)
constexpr int LL_NS = 10;        // sums over frames: 7 hit channels, 3 cursor differences
constexpr int LL_NL = 11;        // loss components: those and the label term
constexpr int LL_HIT = 7;
constexpr int MMD_DMAX = 256;

// v[k][threadIdx.x] of every thread summed over the block, for k < n, in a fixed tree; the totals are s[k * 256]
template <int NV>
__device__ __forceinline__ void block_tree_sum(float (*s)[256]) {
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o) {
#pragma unroll
            for (int k = 0; k < NV; k++) s[k][threadIdx.x] += s[k][threadIdx.x + o];
        }
        __syncthreads();
    }
}

// ---- MMD with the sum of seven inverse multiquadratic kernels, common/wae.py:4-28 ------------------------------------------------
// k(d2) = sum_s C_s / (C_s + d2), C_s = 2 D scale_s;  dk = dk / d(d2)
__device__ __forceinline__ float imq7(float d2, float Cb, float& dk) {
    const float sc[7] = {.1f, .2f, .5f, 1.f, 2.f, 5.f, 10.f};
    float k = 0.f;
    dk = 0.f;
#pragma unroll
    for (int i = 0; i < 7; i++) {
        const float C = Cb * sc[i], inv = 1.f / (C + d2), r = C * inv;
        k += r;
        dk -= r * inv;
    }
    return k;
}

// Block i: row i of z and of p against every row j, squared distances by direct differences.  ws[i] = (sum_{j != i} k(z_i, z_j),
// sum_{j != i} k(p_i, p_j), sum_j k(z_i, p_j));  dz[i] = the gradient of the value with respect to z_i.
__global__ __launch_bounds__(256) void mmd_rows_kernel(const float* __restrict__ z, const float* __restrict__ p, float* __restrict__ ws,
                                                       float* __restrict__ dz, int N, int D) {
    __shared__ float s_zi[MMD_DMAX], s_pi[MMD_DMAX], s_cz[256], s_cp[256], s_red[3][256];
    const int i = blockIdx.x, tid = threadIdx.x;
    if (tid < D) {
        s_zi[tid] = z[(size_t)i * D + tid];
        s_pi[tid] = p[(size_t)i * D + tid];
    }
    __syncthreads();
    const float Cb = 2.f * (float)D;
    float a_zz = 0.f, a_pp = 0.f, a_zp = 0.f, gz = 0.f, gp = 0.f;
    for (int j0 = 0; j0 < N; j0 += 256) {
        const int j = j0 + tid;
        float cz = 0.f, cp = 0.f;
        if (j < N) {
            float dzz = 0.f, dpp = 0.f, dzp = 0.f;
            for (int d = 0; d < D; d++) {
                const float zj = z[(size_t)j * D + d], pj = p[(size_t)j * D + d];
                const float a = s_zi[d] - zj, b = s_pi[d] - pj, c = s_zi[d] - pj;
                dzz += a * a;
                dpp += b * b;
                dzp += c * c;
            }
            a_zp += imq7(dzp, Cb, cp);
            if (j != i) {
                float unused;
                a_zz += imq7(dzz, Cb, cz);
                a_pp += imq7(dpp, Cb, unused);
            }
        }
        s_cz[tid] = cz;
        s_cp[tid] = cp;
        __syncthreads();
        if (tid < D) {
            const int n = N - j0 < 256 ? N - j0 : 256;
            for (int jj = 0; jj < n; jj++) {
                gz += s_cz[jj] * (s_zi[tid] - z[(size_t)(j0 + jj) * D + tid]);
                gp += s_cp[jj] * (s_zi[tid] - p[(size_t)(j0 + jj) * D + tid]);
            }
        }
        __syncthreads();
    }
    // the pair (i, j) is in the zz sum twice; d(d2)/dz_i = 2 (z_i - .)
    if (tid < D) dz[(size_t)i * D + tid] = 4.f / ((float)N * (float)(N - 1)) * gz - 4.f / ((float)N * (float)N) * gp;
    s_red[0][tid] = a_zz;
    s_red[1][tid] = a_pp;
    s_red[2][tid] = a_zp;
    block_tree_sum<3>(s_red);
    if (tid < 3) ws[(size_t)i * 3 + tid] = s_red[tid][0];
}

// out = (value, zz, pp, zp): the N partial rows added in row order
__global__ __launch_bounds__(256) void mmd_finalize_kernel(const float* __restrict__ ws, float* __restrict__ out, int N) {
    __shared__ float s_red[3][256];
    const int tid = threadIdx.x;
    float a[3] = {0.f, 0.f, 0.f};
    for (int r = tid; r < N; r += 256)
        for (int k = 0; k < 3; k++) a[k] += ws[(size_t)r * 3 + k];
    for (int k = 0; k < 3; k++) s_red[k][tid] = a[k];
    block_tree_sum<3>(s_red);
    if (tid == 0) {
        const float n = (float)N, zz = s_red[0][0] / (n * (n - 1.f)), pp = s_red[1][0] / (n * (n - 1.f)), zp = s_red[2][0] / (n * n);
        out[0] = zz + pp - 2.f * zp;
        out[1] = zz;
        out[2] = pp;
        out[3] = zp;
    }
}

__global__ __launch_bounds__(256) void scale_by_kernel(const float* __restrict__ x, const float* __restrict__ g, float* __restrict__ y, long n) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i < n) y[i] = x[i] * g[0];
}

// ---- perturbation of the decoder's inputs, latent/train.py:90-112 -------------------------------------------------------------
// span and start of a row's zeroed frames, in the reference's operation order: every product is rounded to fp32 on its own
__device__ __forceinline__ void mask_span(float u_span, float u_start, float frac, int l, int& start, int& span) {
#pragma clang fp contract(off)
    const float a = u_span * frac;
    span = (int)(a * (float)l);
    const int room = l - span > 1 ? l - span : 1;
    start = (int)(u_start * (float)room);
}

__device__ __forceinline__ float add_scaled(float x, float w, float e) {
#pragma clang fp contract(off)
    const float t = w * e;
    return x + t;
}

__global__ __launch_bounds__(256) void latent_perturb_kernel(const float* __restrict__ z, long zsb, long zse, long zsl,
                                                             const float* __restrict__ s, const float* __restrict__ eps_z,
                                                             const float* __restrict__ eps_s, const float* __restrict__ u_s,
                                                             const float* __restrict__ repl, const float* __restrict__ u_span,
                                                             const float* __restrict__ u_start, float* __restrict__ z_out,
                                                             float* __restrict__ s_out, unsigned char* __restrict__ masked,
                                                             int* __restrict__ start_span, int B2, int E, int l, int S, float s_noise,
                                                             float z_noise, float s_frac, float z_frac, int training) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x, nz = (long)B2 * E * l;
    if (i < nz) {
        const int b = (int)(i / ((long)E * l)), r = (int)(i % ((long)E * l)), e = r / l, t = r % l;
        float v = z[b * zsb + e * zse + t * zsl];
        int st = 0, sp = 0;
        if (training) {
            v = add_scaled(v, z_noise, eps_z[i]);
            if (z_frac > 0.f) {
                mask_span(u_span[b], u_start[b], z_frac, l, st, sp);
                if (t >= st && t < st + sp) v = 0.f;
            }
        }
        z_out[i] = v;
        if (r == 0) {
            start_span[2 * b] = st;
            start_span[2 * b + 1] = sp;
        }
    } else if (i < nz + (long)B2 * S) {
        const long j = i - nz;
        const int b = (int)(j / S), c = (int)(j % S);
        float v = s[(size_t)(b ^ 1) * S + c];          // each half is decoded with the other half's style
        int m = 0;
        if (training) {
            v = add_scaled(v, s_noise, eps_s[j]);
            if (s_frac > 0.f) {
                m = u_s[b] < s_frac;
                if (m) v = repl[j];
            }
        }
        s_out[j] = v;
        if (c == 0) masked[b] = (unsigned char)m;
    }
}

__global__ __launch_bounds__(256) void latent_perturb_bwd_kernel(const float* __restrict__ dz_out, const float* __restrict__ ds_out,
                                                                 const unsigned char* __restrict__ masked,
                                                                 const int* __restrict__ start_span, float* __restrict__ dz,
                                                                 float* __restrict__ ds, int B2, int E, int l, int S) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x, nz = (long)B2 * E * l;
    if (i < nz) {
        const int b = (int)(i / ((long)E * l)), t = (int)(i % l);
        const int st = start_span[2 * b], sp = start_span[2 * b + 1];
        dz[i] = (t >= st && t < st + sp) ? 0.f : dz_out[i];
    } else if (i < nz + (long)B2 * S) {
        const long j = i - nz;
        const int b = (int)(j / S), c = (int)(j % S), o = b ^ 1;       // s[b] went to row o
        ds[j] = masked[o] ? 0.f : ds_out[(size_t)o * S + c];
    }
}

// ---- reconstruction loss, latent/train.py:115-149 ------------------------------------------------------------------------------
__device__ __forceinline__ float xlogx(float t) { return t > 0.f ? t * logf(t) : 0.f; }

// Block (tile, b): LL_T frames of row b.  Partial row: the LL_NS sums of the tile (cursor differences that start in it).
__global__ __launch_bounds__(256) void latent_loss_sums_kernel(const float* __restrict__ logits, const float* __restrict__ chart,
                                                               float* __restrict__ ws, int L) {
    __shared__ float s_red[LL_NS][256];
    const int tid = threadIdx.x, b = blockIdx.y, l = blockIdx.x * LL_T + tid;
    const float* x = logits + (size_t)b * 9 * L;
    const float* y = chart + (size_t)b * 9 * L;
    float acc[LL_NS];
#pragma unroll
    for (int k = 0; k < LL_NS; k++) acc[k] = 0.f;
    if (l < L) {
#pragma unroll
        for (int k = 0; k < LL_HIT; k++) {
            const float v = x[(size_t)k * L + l], t = y[(size_t)k * L + l];
            const float bce = fmaxf(v, 0.f) - v * t + log1pf(expf(-fabsf(v)));
            acc[k] = bce + (xlogx(t) + xlogx(1.f - t));         // minus the soft-target floor -t log t - (1 - t) log(1 - t)
        }
        for (int c = LL_HIT; c < 9; c++) {
            const float* xe = x + (size_t)c * L;
            const float* ye = y + (size_t)c * L;
            const float e0 = xe[l] - ye[l];
            acc[7] += e0 * e0;
            if (l + 1 < L) {
                const float e1 = xe[l + 1] - ye[l + 1], d1 = e1 - e0;
                acc[8] += d1 * d1;
                if (l + 2 < L) {
                    const float e2 = xe[l + 2] - ye[l + 2], d2 = (e2 - e1) - d1;
                    acc[9] += d2 * d2;
                }
            }
        }
    }
#pragma unroll
    for (int k = 0; k < LL_NS; k++) s_red[k][tid] = acc[k];
    block_tree_sum<LL_NS>(s_red);
    if (tid < LL_NS) ws[((size_t)b * gridDim.x + blockIdx.x) * LL_NS + tid] = s_red[tid][0];
}

// One block: the partial rows added in row order, the label term, the EMA of the components, the weighted loss, the 13 logged values
// (the 11 components, s_reg, loss) and the 11 gradient coefficients d loss / d (one term of component i).
__global__ __launch_bounds__(256) void latent_loss_finalize_kernel(const float* __restrict__ ws, int nrows, const float* __restrict__ pred_labels,
                                                                   const float* __restrict__ true_labels,
                                                                   const unsigned char* __restrict__ masked, const float* __restrict__ s_reg,
                                                                   float* __restrict__ loss_ema, unsigned char* __restrict__ ema_init,
                                                                   float* __restrict__ out, float* __restrict__ coef, int B2, int L,
                                                                   float s_reg_weight, int training) {
    __shared__ float s_red[LL_NS + 2][256];
    const int tid = threadIdx.x;
    float acc[LL_NS + 2];
#pragma unroll
    for (int k = 0; k < LL_NS + 2; k++) acc[k] = 0.f;
    for (int r = tid; r < nrows; r += 256)
#pragma unroll
        for (int k = 0; k < LL_NS; k++) acc[k] += ws[(size_t)r * LL_NS + k];
    for (int b = tid; b < B2; b += 256)
        if (!masked[b]) {
            float q = 0.f;
            for (int j = 0; j < 5; j++) {
                const float d = pred_labels[b * 5 + j] - true_labels[b * 5 + j];
                q += d * d;
            }
            acc[LL_NS] += q / 5.f;
            acc[LL_NS + 1] += 1.f;
        }
#pragma unroll
    for (int k = 0; k < LL_NS + 2; k++) s_red[k][tid] = acc[k];
    block_tree_sum<LL_NS + 2>(s_red);
    if (tid == 0) {
        const float wts[LL_NL] = {1.f, 1.f, 1.f, 1.f, 1.f, 1.f, 1.f, 2.f, 2.f, 2.f, 2.f};      // LOSS_COMPONENT_WEIGHTS, train.py:21-33
        float n[LL_NL], g[LL_NL];      // component i = (its sum) / n[i];  d (its sum) / d (a term's argument) carries g[i]
        for (int k = 0; k < LL_HIT; k++) { n[k] = (float)B2 * (float)L; g[k] = 1.f; }
        for (int k = 0; k < 3; k++) { n[LL_HIT + k] = (float)B2 * 2.f * (float)(L - k); g[LL_HIT + k] = 2.f; }
        n[10] = fmaxf(s_red[LL_NS + 1][0], 1.f);
        g[10] = 2.f / 5.f;
        const int first = training && !ema_init[0];
        float loss = 0.f;
        for (int k = 0; k < LL_NL; k++) {
            const float v = s_red[k][0] / n[k];
            float ema = loss_ema[k];
            if (training) {
                ema = first ? v : ema + 0.01f * (v - ema);
                loss_ema[k] = ema;
            }
            const float c = wts[k] / fmaxf(ema, 1e-8f);
            loss += c * v;
            out[k] = v;
            coef[k] = c * g[k] / n[k];
        }
        if (first) ema_init[0] = 1;
        out[LL_NL] = s_reg[0];
        out[LL_NL + 1] = loss + s_reg_weight * s_reg[0];
    }
}

// Block (tile, b): dlogits of LL_T frames of row b under the seed gradient g[0]; the cursor rows read two frames of halo on each side
// from global memory.  Tile 0 also writes the row's dlabels, block (0, 0) the gradient of s_reg.
__global__ __launch_bounds__(256) void latent_loss_grad_kernel(const float* __restrict__ logits, const float* __restrict__ chart,
                                                               const float* __restrict__ pred_labels, const float* __restrict__ true_labels,
                                                               const unsigned char* __restrict__ masked, const float* __restrict__ coef,
                                                               const float* __restrict__ g, float* __restrict__ dlogits,
                                                               float* __restrict__ dlabels, float* __restrict__ ds_reg, int L,
                                                               float s_reg_weight) {
    const int tid = threadIdx.x, b = blockIdx.y, l = blockIdx.x * LL_T + tid;
    const float seed = g[0];
    if (blockIdx.x == 0) {
        if (tid < 5) dlabels[b * 5 + tid] = masked[b] ? 0.f : seed * coef[10] * (pred_labels[b * 5 + tid] - true_labels[b * 5 + tid]);
        if (b == 0 && tid == 5) ds_reg[0] = seed * s_reg_weight;
    }
    if (l >= L) return;
    const float* x = logits + (size_t)b * 9 * L;
    const float* y = chart + (size_t)b * 9 * L;
    float* dx = dlogits + (size_t)b * 9 * L;
#pragma unroll
    for (int k = 0; k < LL_HIT; k++) {
        const float v = x[(size_t)k * L + l], t = y[(size_t)k * L + l];
        const float ev = expf(-fabsf(v)), sg = (v >= 0.f ? 1.f : ev) / (1.f + ev);
        dx[(size_t)k * L + l] = seed * coef[k] * (sg - t);
    }
    const float c0 = coef[7], c1 = coef[8], c2 = coef[9];
    for (int c = LL_HIT; c < 9; c++) {
        const float* xe = x + (size_t)c * L;
        const float* ye = y + (size_t)c * L;
        float e[5];                                         // e[l - 2 .. l + 2], 0 outside the row (never used there)
#pragma unroll
        for (int o = 0; o < 5; o++) {
            const int m = l + o - 2;
            e[o] = (m >= 0 && m < L) ? xe[m] - ye[m] : 0.f;
        }
        float gr = c0 * e[2];
        // first differences d1[j] = e[j + 1] - e[j], j <= L - 2: frame l is the +1 end of d1[l - 1] and the -1 end of d1[l]
        float a1 = 0.f;
        if (l >= 1) a1 += e[2] - e[1];
        if (l + 1 < L) a1 -= e[3] - e[2];
        gr += c1 * a1;
        // second differences d2[j] = e[j + 2] - 2 e[j + 1] + e[j], j <= L - 3
        float a2 = 0.f;
        if (l >= 2) a2 += (e[2] - e[1]) - (e[1] - e[0]);
        if (l >= 1 && l + 1 < L) a2 -= 2.f * ((e[3] - e[2]) - (e[2] - e[1]));
        if (l + 2 < L) a2 += (e[4] - e[3]) - (e[3] - e[2]);
        gr += c2 * a2;
        dx[(size_t)c * L + l] = seed * gr;
    }
}

// ---- validation over ragged groups of whole maps: the reductions above per map, eval only ------------------------------------------
// Map g of a group owns rows 2g and 2g + 1 (its two halves).  Each kernel below is its whole-batch twin restricted to those two rows, with
// the same tiles, the same partial rows and the same order of additions, so a map's values are the bits the twin gives on the two rows alone.

// Block i: row i of z and of p against the two rows of its pair: mmd_rows_kernel with N = 2, without the gradient.
__global__ __launch_bounds__(256) void mmd_pairs_rows_kernel(const float* __restrict__ z, const float* __restrict__ p, float* __restrict__ ws,
                                                             int D) {
    __shared__ float s_zi[MMD_DMAX], s_pi[MMD_DMAX], s_red[3][256];
    const int i = blockIdx.x, tid = threadIdx.x;
    if (tid < D) {
        s_zi[tid] = z[(size_t)i * D + tid];
        s_pi[tid] = p[(size_t)i * D + tid];
    }
    __syncthreads();
    const float Cb = 2.f * (float)D;
    float a_zz = 0.f, a_pp = 0.f, a_zp = 0.f;
    if (tid < 2) {
        const int j = (i & ~1) + tid;
        float dzz = 0.f, dpp = 0.f, dzp = 0.f, unused;
        for (int d = 0; d < D; d++) {
            const float zj = z[(size_t)j * D + d], pj = p[(size_t)j * D + d];
            const float a = s_zi[d] - zj, b = s_pi[d] - pj, c = s_zi[d] - pj;
            dzz += a * a;
            dpp += b * b;
            dzp += c * c;
        }
        a_zp += imq7(dzp, Cb, unused);
        if (j != i) {
            a_zz += imq7(dzz, Cb, unused);
            a_pp += imq7(dpp, Cb, unused);
        }
    }
    s_red[0][tid] = a_zz;
    s_red[1][tid] = a_pp;
    s_red[2][tid] = a_zp;
    block_tree_sum<3>(s_red);
    if (tid < 3) ws[(size_t)i * 3 + tid] = s_red[tid][0];
}

// Block g: out[g] = (value, zz, pp, zp) of the pair, its two partial rows added as mmd_finalize_kernel adds them for N = 2
__global__ __launch_bounds__(256) void mmd_pairs_finalize_kernel(const float* __restrict__ ws, float* __restrict__ out) {
    __shared__ float s_red[3][256];
    const int g = blockIdx.x, tid = threadIdx.x;
    float a[3] = {0.f, 0.f, 0.f};
    if (tid < 2)
        for (int k = 0; k < 3; k++) a[k] += ws[((size_t)2 * g + tid) * 3 + k];
    for (int k = 0; k < 3; k++) s_red[k][tid] = a[k];
    block_tree_sum<3>(s_red);
    if (tid == 0) {
        const float n = 2.f, zz = s_red[0][0] / (n * (n - 1.f)), pp = s_red[1][0] / (n * (n - 1.f)), zp = s_red[2][0] / (n * n);
        out[g * 4 + 0] = zz + pp - 2.f * zp;
        out[g * 4 + 1] = zz;
        out[g * 4 + 2] = pp;
        out[g * 4 + 3] = zp;
    }
}

// Block (tile, b): latent_loss_sums_kernel on the first hlens[b] frames of row b of a batch padded to Hmax; a tile past the row's length
// writes nothing (its partial row is never read) and no frame at or past hlens[b] is loaded.
__global__ __launch_bounds__(256) void latent_loss_maps_sums_kernel(const float* __restrict__ logits, const float* __restrict__ chart,
                                                                    const int* __restrict__ hlens, float* __restrict__ ws, int Hmax) {
    __shared__ float s_red[LL_NS][256];
    const int tid = threadIdx.x, b = blockIdx.y, L = hlens[b], l = blockIdx.x * LL_T + tid;
    if (L < 3 || L > Hmax || (int)blockIdx.x * LL_T >= L) return;
    const float* x = logits + (size_t)b * 9 * Hmax;
    const float* y = chart + (size_t)b * 9 * Hmax;
    float acc[LL_NS];
#pragma unroll
    for (int k = 0; k < LL_NS; k++) acc[k] = 0.f;
    if (l < L) {
#pragma unroll
        for (int k = 0; k < LL_HIT; k++) {
            const float v = x[(size_t)k * Hmax + l], t = y[(size_t)k * Hmax + l];
            const float bce = fmaxf(v, 0.f) - v * t + log1pf(expf(-fabsf(v)));
            acc[k] = bce + (xlogx(t) + xlogx(1.f - t));
        }
        for (int c = LL_HIT; c < 9; c++) {
            const float* xe = x + (size_t)c * Hmax;
            const float* ye = y + (size_t)c * Hmax;
            const float e0 = xe[l] - ye[l];
            acc[7] += e0 * e0;
            if (l + 1 < L) {
                const float e1 = xe[l + 1] - ye[l + 1], d1 = e1 - e0;
                acc[8] += d1 * d1;
                if (l + 2 < L) {
                    const float e2 = xe[l + 2] - ye[l + 2], d2 = (e2 - e1) - d1;
                    acc[9] += d2 * d2;
                }
            }
        }
    }
#pragma unroll
    for (int k = 0; k < LL_NS; k++) s_red[k][tid] = acc[k];
    block_tree_sum<LL_NS>(s_red);
    if (tid < LL_NS) ws[((size_t)b * gridDim.x + blockIdx.x) * LL_NS + tid] = s_red[tid][0];
}

// Block g: latent_loss_finalize_kernel for B2 = 2, L = hlens[2g], training = 0 and no row masked, on the partial rows of rows 2g and 2g + 1
// (nbl of the nbl_max slots of each, row 2g's first).  loss_ema is read, never written.  A pair whose lengths differ or lie outside 3..Hmax
// comes back as NaN.
__global__ __launch_bounds__(256) void latent_loss_maps_finalize_kernel(const float* __restrict__ ws, int nbl_max, const int* __restrict__ hlens,
                                                                        const float* __restrict__ pred_labels,
                                                                        const float* __restrict__ true_labels, const float* __restrict__ s_reg,
                                                                        int s_reg_stride, const float* __restrict__ loss_ema,
                                                                        float* __restrict__ out, int Hmax, float s_reg_weight) {
    __shared__ float s_red[LL_NS + 2][256];
    const int tid = threadIdx.x, g = blockIdx.x, B2 = 2, L = hlens[2 * g];
    if (L < 3 || L > Hmax || hlens[2 * g + 1] != L) {
        if (tid < LL_NL + 2) out[g * (LL_NL + 2) + tid] = __builtin_nanf("");
        return;
    }
    const int nbl = (L + LL_T - 1) / LL_T, nrows = B2 * nbl;
    float acc[LL_NS + 2];
#pragma unroll
    for (int k = 0; k < LL_NS + 2; k++) acc[k] = 0.f;
    for (int r = tid; r < nrows; r += 256) {
        const int b = r / nbl, row = (2 * g + b) * nbl_max + (r - b * nbl);
#pragma unroll
        for (int k = 0; k < LL_NS; k++) acc[k] += ws[(size_t)row * LL_NS + k];
    }
    for (int b = tid; b < B2; b += 256) {
        const float* pl = pred_labels + (size_t)(2 * g + b) * 5;
        const float* tl = true_labels + (size_t)(2 * g + b) * 5;
        float q = 0.f;
        for (int j = 0; j < 5; j++) {
            const float d = pl[j] - tl[j];
            q += d * d;
        }
        acc[LL_NS] += q / 5.f;
        acc[LL_NS + 1] += 1.f;
    }
#pragma unroll
    for (int k = 0; k < LL_NS + 2; k++) s_red[k][tid] = acc[k];
    block_tree_sum<LL_NS + 2>(s_red);
    if (tid == 0) {
        const float wts[LL_NL] = {1.f, 1.f, 1.f, 1.f, 1.f, 1.f, 1.f, 2.f, 2.f, 2.f, 2.f};
        float n[LL_NL];
        for (int k = 0; k < LL_HIT; k++) n[k] = (float)B2 * (float)L;
        for (int k = 0; k < 3; k++) n[LL_HIT + k] = (float)B2 * 2.f * (float)(L - k);
        n[10] = fmaxf(s_red[LL_NS + 1][0], 1.f);
        float* o = out + (size_t)g * (LL_NL + 2);
        const float sr = s_reg[(size_t)g * s_reg_stride];
        float loss = 0.f;
        for (int k = 0; k < LL_NL; k++) {
            const float v = s_red[k][0] / n[k];
            const float c = wts[k] / fmaxf(loss_ema[k], 1e-8f);
            loss += c * v;
            o[k] = v;
        }
        o[LL_NL] = sr;
        o[LL_NL + 1] = loss + s_reg_weight * sr;
    }
}

// ---- eval_metrics per map, latent/train.py:210-255 ---------------------------------------------------------------------------------
constexpr int EV_T = 256;        // frames of one map a block of the first two passes owns
constexpr int EV_NW = 8;         // floats of a tile's partial row: tt, pt, pp, residual, |pixel error|, sum of the true velocity (x, y), total

// true / predicted velocity of channel c (7: x, 8: y) at frame l, in pixels: the difference first (exact for neighbouring positions), one
// product after it
__device__ __forceinline__ float ev_vel(const float* __restrict__ row, int l, float px) { return (row[l + 1] - row[l]) * px; }

__device__ __forceinline__ bool ev_ok(int P, int Pmax) { return P >= 2 && P <= Pmax; }

// Block (tile, g), pass 1: the tile's sums on the onset channel and the cursor channels, and the sum of the true velocity per channel
__global__ __launch_bounds__(256) void latent_eval_sums_kernel(const float* __restrict__ chart, const float* __restrict__ pred,
                                                               const int* __restrict__ plens, float* __restrict__ ws, int Pmax) {
    __shared__ float s_red[7][256];
    const int tid = threadIdx.x, g = blockIdx.y, P = plens[g], l = blockIdx.x * EV_T + tid;
    if (!ev_ok(P, Pmax) || (int)blockIdx.x * EV_T >= P) return;
    const float* y = chart + (size_t)g * 9 * Pmax;
    const float* x = pred + (size_t)g * 9 * Pmax;
    float acc[7] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    if (l < P) {
        const float t = y[l], p = x[l];                     // channel 0: the onset signal
        acc[0] = t * t;
        acc[1] = p * t;
        acc[2] = p * p;
        for (int c = 0; c < 2; c++) {
            const float px = c == 0 ? 512.f : 384.f;
            const float* ye = y + (size_t)(LL_HIT + c) * Pmax;
            const float* xe = x + (size_t)(LL_HIT + c) * Pmax;
            acc[4] += fabsf((xe[l] - ye[l]) * px);
            if (l + 1 < P) {
                const float tv = ev_vel(ye, l, px), r = ev_vel(xe, l, px) - tv;
                acc[3] += r * r;
                acc[5 + c] = tv;
            }
        }
    }
#pragma unroll
    for (int k = 0; k < 7; k++) s_red[k][tid] = acc[k];
    block_tree_sum<7>(s_red);
    if (tid < 7) ws[((size_t)g * gridDim.x + blockIdx.x) * EV_NW + tid] = s_red[tid][0];
}

// Block (tile, g), pass 2: the mean true velocity of the map per channel from pass 1's partial rows (every block of a map adds them in
// the same order), then the tile's squares about it
__global__ __launch_bounds__(256) void latent_eval_total_kernel(const float* __restrict__ chart, const int* __restrict__ plens,
                                                                float* __restrict__ ws, int Pmax) {
    __shared__ float s_red[2][256];
    const int tid = threadIdx.x, g = blockIdx.y, P = plens[g], l = blockIdx.x * EV_T + tid;
    if (!ev_ok(P, Pmax) || (int)blockIdx.x * EV_T >= P) return;
    const int nt = (P + EV_T - 1) / EV_T;
    float* wg = ws + (size_t)g * gridDim.x * EV_NW;
    float a[2] = {0.f, 0.f};
    for (int r = tid; r < nt; r += 256) {
        a[0] += wg[(size_t)r * EV_NW + 5];
        a[1] += wg[(size_t)r * EV_NW + 6];
    }
    s_red[0][tid] = a[0];
    s_red[1][tid] = a[1];
    block_tree_sum<2>(s_red);
    const float mean[2] = {s_red[0][0] / (float)(P - 1), s_red[1][0] / (float)(P - 1)};
    __syncthreads();
    const float* y = chart + (size_t)g * 9 * Pmax;
    float tot = 0.f;
    if (l + 1 < P)
        for (int c = 0; c < 2; c++) {
            const float d = ev_vel(y + (size_t)(LL_HIT + c) * Pmax, l, c == 0 ? 512.f : 384.f) - mean[c];
            tot += d * d;
        }
    s_red[0][tid] = tot;
    block_tree_sum<1>(s_red);
    if (tid == 0) wg[(size_t)blockIdx.x * EV_NW + 7] = s_red[0][0];
}

// Block g: the map's partial rows added in tile order, the label error, and the smallest channel variance of z over the map's own
// latent frames (two passes per channel: the mean, then the squares about it)
__global__ __launch_bounds__(256) void latent_eval_finalize_kernel(const float* __restrict__ ws, int nt_max, const int* __restrict__ plens,
                                                                   const float* __restrict__ z, const int* __restrict__ zlens,
                                                                   const float* __restrict__ pred_labels, const float* __restrict__ true_labels,
                                                                   float* __restrict__ out, int Pmax, int E, int lmax) {
    __shared__ float s_red[6][256];
    const int tid = threadIdx.x, g = blockIdx.x, P = plens[g], zl = zlens[g];
    float* o = out + (size_t)g * 8;
    if (!ev_ok(P, Pmax) || zl < 1 || zl > lmax) {
        if (tid < 8) o[tid] = __builtin_nanf("");
        return;
    }
    const int nt = (P + EV_T - 1) / EV_T;
    const int col[6] = {0, 1, 2, 3, 7, 4};
    float acc[6] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    for (int r = tid; r < nt; r += 256)
#pragma unroll
        for (int k = 0; k < 6; k++) acc[k] += ws[((size_t)g * nt_max + r) * EV_NW + col[k]];
#pragma unroll
    for (int k = 0; k < 6; k++) s_red[k][tid] = acc[k];
    block_tree_sum<6>(s_red);
    if (tid == 0) {
        for (int k = 0; k < 5; k++) o[k] = s_red[k][0];
        o[5] = s_red[5][0] / (2.f * (float)P);
        float q = 0.f;
        for (int j = 0; j < 5; j++) q += fabsf(pred_labels[g * 5 + j] - true_labels[g * 5 + j]);
        o[6] = q / 5.f;
    }
    float vmin = 0.f;
    for (int e = 0; e < E; e++) {
        const float* ze = z + ((size_t)g * E + e) * lmax;
        __syncthreads();
        float a = 0.f;
        for (int t = tid; t < zl; t += 256) a += ze[t];
        s_red[0][tid] = a;
        block_tree_sum<1>(s_red);
        const float mean = s_red[0][0] / (float)zl;
        __syncthreads();
        a = 0.f;
        for (int t = tid; t < zl; t += 256) {
            const float d = ze[t] - mean;
            a += d * d;
        }
        s_red[0][tid] = a;
        block_tree_sum<1>(s_red);
        const float var = s_red[0][0] / (float)(zl - 1);    // unbiased, as torch.var: NaN for a single frame
        if (e == 0 || var < vmin || var != var) vmin = var;  // the minimum; a NaN stays, as in torch.min
    }
    if (tid == 0) o[7] = vmin;
}

}  // namespace

extern "C" int od_latent_loss_block_frames(void) { return LL_T; }

extern "C" int od_latent_loss_ws_floats(int B2, int L) { return B2 * ((L + LL_T - 1) / LL_T) * LL_NS; }

extern "C" int od_mmd_imq(const float* z, const float* prior, float* out, float* dz, float* ws, long ws_floats, int N, int D, void* stream) {
    if (N < 2 || D < 1 || D > MMD_DMAX) return OD_ERR_UNSUPPORTED;
    if (!z || !prior || !out || !dz || !ws || ws_floats < (long)N * 3) return OD_ERR_ARG;
    OD_LAUNCH(mmd_rows_kernel, dim3(N), dim3(256), 0, (hipStream_t)stream, z, prior, ws, dz, N, D);
    OD_LAUNCH(mmd_finalize_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, ws, out, N);
    OD_CHECK_LAUNCH();
    return 0;
}

extern "C" int od_scale_by(const float* x, const float* g, float* y, long n, void* stream) {
    if (n <= 0 || !x || !g || !y) return OD_ERR_ARG;
    OD_LAUNCH(scale_by_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, x, g, y, n);
    OD_CHECK_LAUNCH();
    return 0;
}

extern "C" int od_latent_perturb(const float* z, long zsb, long zse, long zsl, const float* s, const float* eps_z, const float* eps_s,
                                 const float* u_s, const float* repl, const float* u_span, const float* u_start, float* z_out,
                                 float* s_out, void* masked, void* start_span, int B2, int E, int l, int S, float s_noise, float z_noise,
                                 float s_mask_frac, float z_mask_frac, int training, void* stream) {
    if (B2 <= 0 || B2 % 2 || E <= 0 || l <= 0 || S <= 0 || !z || !s || !z_out || !s_out || !masked || !start_span) return OD_ERR_ARG;
    if (training && (!eps_z || !eps_s || (s_mask_frac > 0.f && (!u_s || !repl)) || (z_mask_frac > 0.f && (!u_span || !u_start))))
        return OD_ERR_ARG;
    const long n = (long)B2 * E * l + (long)B2 * S;
    OD_LAUNCH(latent_perturb_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, z, zsb, zse, zsl, s, eps_z,
              eps_s, u_s, repl, u_span, u_start, z_out, s_out, (unsigned char*)masked, (int*)start_span, B2, E, l, S, s_noise, z_noise,
              s_mask_frac, z_mask_frac, training);
    OD_CHECK_LAUNCH();
    return 0;
}

extern "C" int od_latent_perturb_bwd(const float* dz_out, const float* ds_out, const void* masked, const int* start_span, float* dz,
                                     float* ds, int B2, int E, int l, int S, void* stream) {
    if (B2 <= 0 || B2 % 2 || E <= 0 || l <= 0 || S <= 0 || !dz_out || !ds_out || !masked || !start_span || !dz || !ds) return OD_ERR_ARG;
    const long n = (long)B2 * E * l + (long)B2 * S;
    OD_LAUNCH(latent_perturb_bwd_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, dz_out, ds_out,
              (const unsigned char*)masked, start_span, dz, ds, B2, E, l, S);
    OD_CHECK_LAUNCH();
    return 0;
}

extern "C" int od_latent_loss(const float* logits, const float* chart, const float* pred_labels, const float* true_labels,
                              const void* masked, const float* s_reg, float* loss_ema, void* ema_init, float* out, float* coef, float* ws,
                              long ws_floats, int B2, int L, float s_reg_weight, int training, void* stream) {
    if (L < 3) return OD_ERR_UNSUPPORTED;                  // the second difference needs three frames
    if (B2 <= 0 || !logits || !chart || !pred_labels || !true_labels || !masked || !s_reg || !loss_ema || !ema_init || !out || !coef || !ws)
        return OD_ERR_ARG;
    const int nbl = (L + LL_T - 1) / LL_T;
    if (ws_floats < (long)B2 * nbl * LL_NS) return OD_ERR_ARG;
    OD_LAUNCH(latent_loss_sums_kernel, dim3(nbl, B2), dim3(256), 0, (hipStream_t)stream, logits, chart, ws, L);
    OD_LAUNCH(latent_loss_finalize_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, ws, B2 * nbl, pred_labels, true_labels,
              (const unsigned char*)masked, s_reg, loss_ema, (unsigned char*)ema_init, out, coef, B2, L, s_reg_weight, training);
    OD_CHECK_LAUNCH();
    return 0;
}

extern "C" int od_mmd_imq_pairs(const float* s, const float* prior, float* out, float* ws, long ws_floats, int G, int S, void* stream) {
    if (G < 1 || S < 1 || S > MMD_DMAX) return OD_ERR_UNSUPPORTED;
    if (!s || !prior || !out || !ws || ws_floats < (long)G * 6) return OD_ERR_ARG;
    OD_LAUNCH(mmd_pairs_rows_kernel, dim3(2 * G), dim3(256), 0, (hipStream_t)stream, s, prior, ws, S);
    OD_LAUNCH(mmd_pairs_finalize_kernel, dim3(G), dim3(256), 0, (hipStream_t)stream, ws, out);
    OD_CHECK_LAUNCH();
    return 0;
}

extern "C" int od_latent_loss_maps(const float* logits, const float* chart, const int* hlens, const float* pred_labels,
                                   const float* true_labels, const float* s_reg, int s_reg_stride, const float* loss_ema, float* out,
                                   float* ws, long ws_floats, int G, int Hmax, float s_reg_weight, void* stream) {
    if (Hmax < 3) return OD_ERR_UNSUPPORTED;
    if (G < 1 || s_reg_stride < 1 || !logits || !chart || !hlens || !pred_labels || !true_labels || !s_reg || !loss_ema || !out || !ws)
        return OD_ERR_ARG;
    const int nbl = (Hmax + LL_T - 1) / LL_T;
    if (ws_floats < (long)2 * G * nbl * LL_NS) return OD_ERR_ARG;
    OD_LAUNCH(latent_loss_maps_sums_kernel, dim3(nbl, 2 * G), dim3(256), 0, (hipStream_t)stream, logits, chart, hlens, ws, Hmax);
    OD_LAUNCH(latent_loss_maps_finalize_kernel, dim3(G), dim3(256), 0, (hipStream_t)stream, ws, nbl, hlens, pred_labels, true_labels, s_reg,
              s_reg_stride, loss_ema, out, Hmax, s_reg_weight);
    OD_CHECK_LAUNCH();
    return 0;
}

extern "C" int od_latent_eval_maps_ws_floats(int G, int Pmax) { return G * ((Pmax + EV_T - 1) / EV_T) * EV_NW; }

extern "C" int od_latent_eval_maps(const float* chart, const float* pred_chart, const int* plens, const float* z, const int* zlens,
                                   const float* pred_labels, const float* true_labels, float* out, float* ws, long ws_floats, int G,
                                   int Pmax, int E, int lmax, void* stream) {
    if (G < 1 || Pmax < 2 || E < 1 || lmax < 1 || !chart || !pred_chart || !plens || !z || !zlens || !pred_labels || !true_labels || !out || !ws)
        return OD_ERR_ARG;
    const int nt = (Pmax + EV_T - 1) / EV_T;
    if (ws_floats < (long)G * nt * EV_NW) return OD_ERR_ARG;
    OD_LAUNCH(latent_eval_sums_kernel, dim3(nt, G), dim3(256), 0, (hipStream_t)stream, chart, pred_chart, plens, ws, Pmax);
    OD_LAUNCH(latent_eval_total_kernel, dim3(nt, G), dim3(256), 0, (hipStream_t)stream, chart, plens, ws, Pmax);
    OD_LAUNCH(latent_eval_finalize_kernel, dim3(G), dim3(256), 0, (hipStream_t)stream, ws, nt, plens, z, zlens, pred_labels, true_labels, out,
              Pmax, E, lmax);
    OD_CHECK_LAUNCH();
    return 0;
}

extern "C" int od_latent_loss_bwd(const float* logits, const float* chart, const float* pred_labels, const float* true_labels,
                                  const void* masked, const float* coef, const float* g, float* dlogits, float* dlabels, float* ds_reg,
                                  int B2, int L, float s_reg_weight, void* stream) {
    if (L < 3) return OD_ERR_UNSUPPORTED;
    if (B2 <= 0 || !logits || !chart || !pred_labels || !true_labels || !masked || !coef || !g || !dlogits || !dlabels || !ds_reg)
        return OD_ERR_ARG;
    OD_LAUNCH(latent_loss_grad_kernel, dim3((L + LL_T - 1) / LL_T, B2), dim3(256), 0, (hipStream_t)stream, logits, chart, pred_labels,
              true_labels, (const unsigned char*)masked, coef, g, dlogits, dlabels, ds_reg, L, s_reg_weight);
    OD_CHECK_LAUNCH();
    return 0;
}
