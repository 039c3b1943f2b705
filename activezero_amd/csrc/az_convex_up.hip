// K15 / K16 -- RAFT-Stereo's prediction head: the convex-combination upsampling of the 1/f-resolution flow
// (reference nets/raft/raft_stereo.py:74-86 `RAFTStereo.upsample_flow`) and one prediction's term of the sequence loss
// (utils/losses.py:34-69 `sequence_loss`).
//
// The reference softmaxes the [N, 9 f f, h, w] mask over a strided dimension and materialises the result, unfolds the
// flow, materialises the 9 f f-channel product, reduces it and permutes -- and autograd keeps both 9 f f-channel tensors
// per GRU iteration.  Here a pixel's 9 logits are read once; softmax, the 3x3 unfold, the weighted sum and the pixel
// shuffle happen in registers; the backward recomputes the softmax from the mask, so nothing of mask size is saved.
// HBM-bound: forward = mask + flow + output, backward = mask + g_mask + g_up + the small tensors.
//
// Mask channel index: k f f + i f + j with k = ky 3 + kx; thread = (coarse pixel p = y w + x, sub-row i): for each j its
// nine loads are coalesced row segments of nine channel planes, its f outputs one vector store.
#include <hip/hip_fp16.h>

#include "az_block_reduce.h"
#include "az_common.h"

#define CU_BLOCK 256
#define SL_BLOCK 256

__device__ __forceinline__ float cu_ld(const float *p, size_t o) { return p[o]; }
__device__ __forceinline__ float cu_ld(const __half *p, size_t o) { return __half2float(p[o]); }
__device__ __forceinline__ void cu_st(float *p, size_t o, float v) { p[o] = v; }

__device__ __forceinline__ void cu_st_f64(float *p, size_t o, double v) { p[o] = (float)v; }
__device__ __forceinline__ void cu_st_f64(__half *p, size_t o, double v) { reinterpret_cast<_Float16 *>(p)[o] = (_Float16)v; }

// the 3x3 neighbourhood of flow[n, d, y, x] for d < DO; out-of-range neighbours are zero (F.unfold(..., padding=1))
template <int DO>
__device__ __forceinline__ void cu_taps(float (&fl)[DO][9], const float *__restrict__ flow, int n, int D, int h, int w,
                                        int y, int x) {
#pragma unroll
    for (int d = 0; d < DO; ++d)
#pragma unroll
        for (int k = 0; k < 9; ++k) {
            const int yy = y + k / 3 - 1, xx = x + k % 3 - 1;
            const bool ok = yy >= 0 && yy < h && xx >= 0 && xx < w;
            fl[d][k] = ok ? flow[((size_t)(n * D + d) * h + yy) * w + xx] : 0.f;
        }
}

// (In the multiply-adds below the factor that hipcc broadcasts when it packs two of them into a v_pk_fma_f32 is written
// FIRST: as the second factor it can land in the high register of a pair selected for src1, the form tools/isa_lint.py
// keeps out of the library -- see az_conv3d_c1.hip.)
// e[k] = exp(m[k] - max m), returns their sum (>= 1).  Logits of +-80 (fp32) or +-60000 (fp16) stay finite: the
// largest argument is 0, the smallest underflows to 0.
__device__ __forceinline__ float cu_softmax_terms(float (&e)[9], const float (&m)[9]) {
    float mx = m[0];
#pragma unroll
    for (int k = 1; k < 9; ++k) mx = fmaxf(mx, m[k]);
    float s = 0.f;
#pragma unroll
    for (int k = 0; k < 9; ++k) {
        e[k] = __expf(m[k] - mx);
        s += e[k];
    }
    return s;
}

// exp(x) for x <= 0 in fp64 to ~1e-11 relative (range reduction by ln 2 in two parts, degree-9 Taylor polynomial on
// |r| <= 0.35, v_ldexp_f64): the softmax terms of the fp16 backward, see convex_up_bwd_kernel
__device__ __forceinline__ double cu_exp_f64(double x) {
    x = x < -700.0 ? -700.0 : x;  // 2^-1010 stays normal; a NaN passes through
    const double n = rint(x * 1.4426950408889634);
    double r = fma(n, -6.93147180369123816490e-01, x);
    r = fma(n, -1.90821492927058770002e-10, r);
    double q = 1.0 / 362880.0;
    q = fma(q, r, 1.0 / 40320.0);
    q = fma(q, r, 1.0 / 5040.0);
    q = fma(q, r, 1.0 / 720.0);
    q = fma(q, r, 1.0 / 120.0);
    q = fma(q, r, 1.0 / 24.0);
    q = fma(q, r, 1.0 / 6.0);
    q = fma(q, r, 0.5);
    q = fma(q, r, 1.0);
    q = fma(q, r, 1.0);
    return ldexp(q, (int)n);
}

// up[n, d, y f + i, x f + j] = scale * sum_k softmax_k(mask[n, k, i, j, y, x]) flow[n, d, y + ky - 1, x + kx - 1]
// (scale = +-f: a power of two, so scaling the sum equals summing the scaled flow).  grid (hw / 256, f, N)
template <int F, int DO, typename MT>
__global__ void __launch_bounds__(CU_BLOCK)
convex_up_fwd_kernel(float *__restrict__ up, const float *__restrict__ flow, const MT *__restrict__ mask, int D, int h,
                     int w, float scale) {
    const int hw = h * w;
    const int p = blockIdx.x * CU_BLOCK + threadIdx.x;
    if (p >= hw) return;
    const int i = blockIdx.y, n = blockIdx.z;
    const int y = p / w, x = p - y * w;
    float fl[DO][9];
    cu_taps<DO>(fl, flow, n, D, h, w, y, x);
    const MT *mp = mask + ((size_t)n * 9 * F * F + (size_t)i * F) * hw + p;
    float out[DO][F];
#pragma unroll
    for (int j = 0; j < F; ++j) {
        float m[9], e[9];
#pragma unroll
        for (int k = 0; k < 9; ++k) m[k] = cu_ld(mp, (size_t)(k * F * F + j) * hw);
        const float s = cu_softmax_terms(e, m);
#pragma unroll
        for (int d = 0; d < DO; ++d) {
            float a = 0.f;
#pragma unroll
            for (int k = 0; k < 9; ++k) a = fmaf(fl[d][k], e[k], a);
            out[d][j] = scale * (a / s);
        }
    }
#pragma unroll
    for (int d = 0; d < DO; ++d) {
        float4 *o = reinterpret_cast<float4 *>(up + ((size_t)(n * DO + d) * (h * F) + (size_t)y * F + i) * ((size_t)w * F) +
                                               (size_t)x * F);
#pragma unroll
        for (int q = 0; q < F / 4; ++q) o[q] = make_float4(out[d][4 * q], out[d][4 * q + 1], out[d][4 * q + 2], out[d][4 * q + 3]);
    }
}

// g_mask[n, k, i, j, y, x] = p_k (G_k - sum_m p_m G_m), G_k = scale sum_d g_up[n, d, y f + i, x f + j] flow_k[d]; and the
// tap sums tsum[n, d, k, y, x] = scale sum_ij p_k g_up: the block's f waves (one per sub-row i) each sum over j in
// registers, and the f partial sums are added in LDS in the fixed order i = 0 .. f-1.  grid (hw / 64, N), 64 f threads.
// G_k is taken relative to the tap with the largest logit, G'_k = scale sum_d g (flow_k - flow_kmax): the bracket does
// not change (the p_m sum to 1), but at a near-one-hot pixel G_kmax - sum_m p_m G_m is a difference of two numbers of
// size |G| whose exact value is ~p_other |G|; with G'_kmax = 0 it is a short sum of small terms instead.
// With an fp16 mask g_mask is written in fp16, whose subnormals resolve 6e-8 ABSOLUTE: where the bracket of a
// near-uniform pixel happens to cancel to ~1e-4 |G| an fp32 evaluation (p_m known to 1e-7, the bracket to ~1e-7 |G|) is
// several fp16 ulp off.  That instantiation therefore evaluates the softmax terms and the bracket in fp64 (~25 fp64
// instructions per mask element; its mask traffic is half the fp32 one's) and rounds once, to fp16.
template <int F, int DO, typename MT>
__global__ void __launch_bounds__(64 * F)
convex_up_bwd_kernel(MT *__restrict__ gmask, float *__restrict__ tsum, const float *__restrict__ gup,
                     const float *__restrict__ flow, const MT *__restrict__ mask, int D, int h, int w, float scale) {
    __shared__ float red[F][DO * 9][64];
    const int hw = h * w;
    const int lane = threadIdx.x & 63, i = threadIdx.x >> 6, n = blockIdx.y;
    const int p = blockIdx.x * 64 + lane;
    float t[DO][9];
#pragma unroll
    for (int d = 0; d < DO; ++d)
#pragma unroll
        for (int k = 0; k < 9; ++k) t[d][k] = 0.f;
    if (p < hw) {
        const int y = p / w, x = p - y * w;
        float fl[DO][9];
        cu_taps<DO>(fl, flow, n, D, h, w, y, x);
        float g[DO][F];
#pragma unroll
        for (int d = 0; d < DO; ++d) {
            const float4 *gp = reinterpret_cast<const float4 *>(
                gup + ((size_t)(n * DO + d) * (h * F) + (size_t)y * F + i) * ((size_t)w * F) + (size_t)x * F);
#pragma unroll
            for (int q = 0; q < F / 4; ++q) {
                const float4 v = gp[q];
                g[d][4 * q] = v.x, g[d][4 * q + 1] = v.y, g[d][4 * q + 2] = v.z, g[d][4 * q + 3] = v.w;
            }
        }
        const size_t base = ((size_t)n * 9 * F * F + (size_t)i * F) * hw + p;
        // fp32: fully unrolled, the loads of all j in flight.  fp16 (fp64 temporaries): a real loop, one j's registers at a
        // time -- unrolled it needs more than 256 registers; occupancy hides the load latency instead
        constexpr int UNROLL_J = sizeof(MT) == 2 ? 1 : F;
#pragma unroll UNROLL_J
        for (int j = 0; j < F; ++j) {
            float m[9], e[9], gj[DO];
#pragma unroll
            for (int k = 0; k < 9; ++k) m[k] = cu_ld(mask, base + (size_t)(k * F * F + j) * hw);
#pragma unroll
            for (int d = 0; d < DO; ++d) {  // g[d][j] by selects: a run-time index would put g in scratch memory
                gj[d] = g[d][0];
#pragma unroll
                for (int jj = 1; jj < F; ++jj) gj[d] = j == jj ? g[d][jj] : gj[d];
            }
            float mx = m[0], fm[DO];
#pragma unroll
            for (int d = 0; d < DO; ++d) fm[d] = fl[d][0];
#pragma unroll
            for (int k = 1; k < 9; ++k) {
                const bool up = m[k] > mx;
                mx = up ? m[k] : mx;
#pragma unroll
                for (int d = 0; d < DO; ++d) fm[d] = up ? fl[d][k] : fm[d];
            }
            if constexpr (sizeof(MT) == 2) {
                double ed[9], Gd[9], sd = 0.0, Td = 0.0;
#pragma unroll
                for (int k = 0; k < 9; ++k) {
                    ed[k] = cu_exp_f64((double)m[k] - (double)mx);  // fp16 values: the difference is exact in fp64
                    sd += ed[k];
                    double a = 0.0;
#pragma unroll
                    for (int d = 0; d < DO; ++d) a = fma((double)gj[d], (double)fl[d][k] - (double)fm[d], a);
                    Gd[k] = a;
                    Td = fma(ed[k], a, Td);
                }
                const double invd = 1.0 / sd;
                const double Sd = Td * invd;
#pragma unroll
                for (int k = 0; k < 9; ++k) {
                    const double pk = ed[k] * invd;
                    e[k] = (float)pk;
#pragma unroll
                    for (int d = 0; d < DO; ++d) t[d][k] = fmaf(gj[d], e[k], t[d][k]);
                    // one rounding, fp64 -> fp16 (through fp32 the two roundings could add up to more than half an ulp)
                    cu_st_f64(gmask, base + (size_t)(k * F * F + j) * hw, (double)scale * pk * (Gd[k] - Sd));
                }
            } else {
                const float inv = 1.f / cu_softmax_terms(e, m);
                float G[9], S = 0.f;
#pragma unroll
                for (int k = 0; k < 9; ++k) {
                    e[k] = inv * e[k];  // p_k
                    float a = 0.f;
#pragma unroll
                    for (int d = 0; d < DO; ++d) {
                        a = fmaf(gj[d], fl[d][k] - fm[d], a);
                        t[d][k] = fmaf(gj[d], e[k], t[d][k]);
                    }
                    G[k] = scale * a;
                    S = fmaf(e[k], G[k], S);
                }
#pragma unroll
                for (int k = 0; k < 9; ++k) cu_st(gmask, base + (size_t)(k * F * F + j) * hw, e[k] * (G[k] - S));
            }
        }
    }
#pragma unroll
    for (int d = 0; d < DO; ++d)
#pragma unroll
        for (int k = 0; k < 9; ++k) red[i][d * 9 + k][lane] = t[d][k];
    __syncthreads();
    for (int e = threadIdx.x; e < DO * 9 * 64; e += 64 * F) {
        const int q = e >> 6, l = e & 63;
        const int pp = blockIdx.x * 64 + l;
        if (pp >= hw) continue;
        float s = red[0][q][l];
#pragma unroll
        for (int ii = 1; ii < F; ++ii) s += red[ii][q][l];
        tsum[((size_t)n * DO * 9 + q) * hw + pp] = scale * s;
    }
}

// g_flow[n, d, y, x] = sum_k tsum[n, d, k, y - ky + 1, x - kx + 1] (the pixels whose tap k reads this flow pixel), in the
// fixed order k = 0 .. 8; channels >= DO are zero
__global__ void __launch_bounds__(CU_BLOCK)
convex_up_gather_kernel(float *__restrict__ gflow, const float *__restrict__ tsum, int N, int D, int DO, int h, int w) {
    const long long total = (long long)N * D * h * w;
    const long long idx = (long long)blockIdx.x * CU_BLOCK + threadIdx.x;
    if (idx >= total) return;
    const int x = (int)(idx % w), y = (int)(idx / w % h), d = (int)(idx / ((long long)w * h) % D);
    const int n = (int)(idx / ((long long)w * h * D));
    float s = 0.f;
    if (d < DO) {
#pragma unroll
        for (int k = 0; k < 9; ++k) {
            const int yy = y - (k / 3 - 1), xx = x - (k % 3 - 1);
            if (yy >= 0 && yy < h && xx >= 0 && xx < w) s += tsum[(((size_t)(n * DO + d) * 9 + k) * h + yy) * w + xx];
        }
    }
    gflow[idx] = s;
}

static int cu_check(int N, int D, int D_out, int h, int w, int factor, int mask_channels, int sign) {
    AZ_REQUIRE(N >= 0 && D >= 1 && h >= 0 && w >= 0 && factor >= 1 && mask_channels >= 1);
    AZ_REQUIRE(D_out >= 1 && D_out <= D);
    AZ_REQUIRE(sign == 1 || sign == -1);
    if ((factor != 4 && factor != 8) || D > 2 || mask_channels != 9 * factor * factor) return AZ_EUNSUPPORTED;
    if (N > 65535 || (long long)h * w > (1LL << 30) / (factor * factor)) return AZ_EUNSUPPORTED;  // grid.z; int pixel index
    return AZ_OK;
}

template <int F, int DO, typename MT>
static void cu_launch_fwd(float *up, const float *flow, const void *mask, int N, int D, int h, int w, float scale,
                          hipStream_t st) {
    const dim3 grid((unsigned)(((long long)h * w + CU_BLOCK - 1) / CU_BLOCK), F, N);
    hipLaunchKernelGGL((convex_up_fwd_kernel<F, DO, MT>), grid, dim3(CU_BLOCK), 0, st, up, flow,
                       static_cast<const MT *>(mask), D, h, w, scale);
}

template <int F, int DO, typename MT>
static void cu_launch_bwd(void *gmask, float *tsum, const float *gup, const float *flow, const void *mask, int N, int D,
                          int h, int w, float scale, hipStream_t st) {
    const dim3 grid((unsigned)(((long long)h * w + 63) / 64), N);
    hipLaunchKernelGGL((convex_up_bwd_kernel<F, DO, MT>), grid, dim3(64 * F), 0, st, static_cast<MT *>(gmask), tsum, gup,
                       flow, static_cast<const MT *>(mask), D, h, w, scale);
}

#define CU_DISPATCH(CALL, ...)                                                          \
    do {                                                                                \
        if (factor == 4 && D_out == 1 && !mask_f16) CALL<4, 1, float>(__VA_ARGS__);      \
        else if (factor == 4 && D_out == 2 && !mask_f16) CALL<4, 2, float>(__VA_ARGS__); \
        else if (factor == 8 && D_out == 1 && !mask_f16) CALL<8, 1, float>(__VA_ARGS__); \
        else if (factor == 8 && D_out == 2 && !mask_f16) CALL<8, 2, float>(__VA_ARGS__); \
        else if (factor == 4 && D_out == 1) CALL<4, 1, __half>(__VA_ARGS__);             \
        else if (factor == 4 && D_out == 2) CALL<4, 2, __half>(__VA_ARGS__);             \
        else if (factor == 8 && D_out == 1) CALL<8, 1, __half>(__VA_ARGS__);             \
        else CALL<8, 2, __half>(__VA_ARGS__);                                            \
    } while (0)

extern "C" int az_convex_up_fwd(float *up, const float *flow, const void *mask, int mask_f16, int N, int D, int D_out,
                                int h, int w, int factor, int mask_channels, int sign, void *stream) {
    AZ_REQUIRE_PTR(up); AZ_REQUIRE_PTR(flow); AZ_REQUIRE_PTR(mask);
    AZ_REQUIRE(reinterpret_cast<uintptr_t>(up) % 16 == 0);  // written as float4
    const int rc = cu_check(N, D, D_out, h, w, factor, mask_channels, sign);
    if (rc != AZ_OK) return rc;
    if (N == 0 || h == 0 || w == 0) return AZ_OK;
    const float scale = (float)(sign * factor);
    CU_DISPATCH(cu_launch_fwd, up, flow, mask, N, D, h, w, scale, az_stream(stream));
    return az_launch_status();
}

extern "C" long long az_convex_up_bwd_workspace(int N, int D_out, int h, int w) {
    if (N < 0 || D_out < 1 || h < 0 || w < 0) return AZ_EINVAL;
    return (long long)N * D_out * 9 * h * w * (long long)sizeof(float);
}

extern "C" int az_convex_up_bwd(void *g_mask, float *g_flow, void *workspace, long long workspace_bytes,
                                const float *g_up, const float *flow, const void *mask, int mask_f16, int N, int D,
                                int D_out, int h, int w, int factor, int mask_channels, int sign, void *stream) {
    AZ_REQUIRE_PTR(g_mask); AZ_REQUIRE_PTR(g_flow); AZ_REQUIRE_PTR(g_up); AZ_REQUIRE_PTR(flow); AZ_REQUIRE_PTR(mask);
    AZ_REQUIRE(reinterpret_cast<uintptr_t>(g_up) % 16 == 0);  // read as float4
    const int rc = cu_check(N, D, D_out, h, w, factor, mask_channels, sign);
    if (rc != AZ_OK) return rc;
    if (N == 0 || h == 0 || w == 0) return AZ_OK;
    AZ_REQUIRE_PTR(workspace);
    if (workspace_bytes < az_convex_up_bwd_workspace(N, D_out, h, w)) return AZ_EWORKSPACE;
    const float scale = (float)(sign * factor);
    float *tsum = static_cast<float *>(workspace);
    CU_DISPATCH(cu_launch_bwd, g_mask, tsum, g_up, flow, mask, N, D, h, w, scale, az_stream(stream));
    if (az_launch_status() != AZ_OK) return AZ_ELAUNCH;
    const long long total = (long long)N * D * h * w;
    hipLaunchKernelGGL(convex_up_gather_kernel, dim3((unsigned)((total + CU_BLOCK - 1) / CU_BLOCK)), dim3(CU_BLOCK), 0,
                       az_stream(stream), g_flow, tsum, N, D, D_out, h, w);
    return az_launch_status();
}

// ---- K16: one prediction's term of sequence_loss ------------------------------------------------------------
// valid pixel: valid >= 0.5 (a byte map: != 0) and |gt| < max_flow (losses.py:45-48, one-channel flow)
template <typename VT>
__device__ __forceinline__ bool sl_valid(const VT *valid, float gt, float max_flow, long long i) {
    return (float)valid[i] >= 0.5f && fabsf(gt) < max_flow;
}

// acc[0] += sum |pred - tsign gt| over valid pixels, acc[1] += count, acc[2] += number of non-finite pred (all pixels)
template <typename VT>
__global__ void __launch_bounds__(SL_BLOCK)
seq_loss_fwd_kernel(double *__restrict__ acc, const float *__restrict__ pred, const float *__restrict__ gt,
                    const VT *__restrict__ valid, float max_flow, float tsign, long long n) {
    double v[3] = {0.0, 0.0, 0.0};
    for (long long i = (long long)blockIdx.x * SL_BLOCK + threadIdx.x; i < n; i += (long long)gridDim.x * SL_BLOCK) {
        const float p = pred[i], g = gt[i];
        if ((__float_as_uint(p) & 0x7f800000u) == 0x7f800000u) v[2] += 1.0;
        if (!sl_valid(valid, g, max_flow, i)) continue;
        v[0] += fabsf(p - tsign * g);
        v[1] += 1.0;
    }
    az_block_sum_f64<3, SL_BLOCK>(v, acc);
}

// g = weight gloss / count sign(pred - tsign gt) on valid pixels, 0 elsewhere; sign(0) = 0 as abs's autograd has it
template <typename VT>
__global__ void __launch_bounds__(SL_BLOCK)
seq_loss_bwd_kernel(float *__restrict__ gout, const float *__restrict__ pred, const float *__restrict__ gt,
                    const VT *__restrict__ valid, float max_flow, float tsign, const float *__restrict__ gloss,
                    const double *__restrict__ acc, float weight, long long n) {
    const float s = weight * gloss[0] / (float)acc[1];
    for (long long i = (long long)blockIdx.x * SL_BLOCK + threadIdx.x; i < n; i += (long long)gridDim.x * SL_BLOCK) {
        const float g = gt[i];
        const float d = pred[i] - tsign * g;
        const float sg = d > 0.f ? s : d < 0.f ? -s : 0.f * d;  // NaN stays NaN
        gout[i] = sl_valid(valid, g, max_flow, i) ? sg : 0.f;
    }
}

static unsigned sl_reduce_grid(long long n) {
    const unsigned g = az_grid_for(n, SL_BLOCK);
    return g > 1024u ? 1024u : g;
}

extern "C" int az_seq_loss_fwd(double *acc3, const float *pred, const float *gt, const void *valid, int valid_u8,
                               float max_flow, int tsign, long long n, void *stream) {
    AZ_REQUIRE_PTR(acc3); AZ_REQUIRE_PTR(pred); AZ_REQUIRE_PTR(gt); AZ_REQUIRE_PTR(valid);
    AZ_REQUIRE(n >= 0 && (tsign == 1 || tsign == -1));
    if (n == 0) return AZ_OK;
    if (valid_u8)
        hipLaunchKernelGGL(seq_loss_fwd_kernel<unsigned char>, dim3(sl_reduce_grid(n)), dim3(SL_BLOCK), 0, az_stream(stream),
                           acc3, pred, gt, static_cast<const unsigned char *>(valid), max_flow, (float)tsign, n);
    else
        hipLaunchKernelGGL(seq_loss_fwd_kernel<float>, dim3(sl_reduce_grid(n)), dim3(SL_BLOCK), 0, az_stream(stream), acc3,
                           pred, gt, static_cast<const float *>(valid), max_flow, (float)tsign, n);
    return az_launch_status();
}

extern "C" int az_seq_loss_bwd(float *g_pred, const float *pred, const float *gt, const void *valid, int valid_u8,
                               float max_flow, int tsign, const float *gloss, const double *acc3, float weight,
                               long long n, void *stream) {
    AZ_REQUIRE_PTR(g_pred); AZ_REQUIRE_PTR(pred); AZ_REQUIRE_PTR(gt); AZ_REQUIRE_PTR(valid);
    AZ_REQUIRE_PTR(gloss); AZ_REQUIRE_PTR(acc3);
    AZ_REQUIRE(n >= 0 && (tsign == 1 || tsign == -1));
    if (n == 0) return AZ_OK;
    if (valid_u8)
        hipLaunchKernelGGL(seq_loss_bwd_kernel<unsigned char>, dim3(az_grid_for(n, SL_BLOCK)), dim3(SL_BLOCK), 0,
                           az_stream(stream), g_pred, pred, gt, static_cast<const unsigned char *>(valid), max_flow,
                           (float)tsign, gloss, acc3, weight, n);
    else
        hipLaunchKernelGGL(seq_loss_bwd_kernel<float>, dim3(az_grid_for(n, SL_BLOCK)), dim3(SL_BLOCK), 0, az_stream(stream),
                           g_pred, pred, gt, static_cast<const float *>(valid), max_flow, (float)tsign, gloss, acc3, weight,
                           n);
    return az_launch_status();
}
