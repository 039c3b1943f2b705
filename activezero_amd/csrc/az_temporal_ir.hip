// K17 -- temporal IR pattern on the GPU: reference tools/temporal_ir.py:91-114, the offline pass that
// writes every real scene's "temporal" pattern (the target of the patch reprojection loss, K8) from the T = 7
// projector exposures of one view, with its helper get_smoothed_ir_pattern (:35-40):
//     slope = sum (x - xbar)(y - ybar) / sum (x - xbar)^2        per pixel, x = 0..T-1
//     diff  = |fit[T-1] - fit[0]| / 255 = |slope (T - 1)| / 255, min-max normalised over the image
//     ir    = (diff - cv2.blur(diff, (ks, ks)) > threshold) ? 1 : 0
// cv2.blur is the normalised ks x ks box filter with cv2's default border BORDER_REFLECT_101 (index -i -> i,
// H-1+i -> H-1-i: the edge pixel is not repeated); cv2 is absent here, the filter is restated from its published
// definition (tests/_temporal_ir_ref.py says the same of the fp64 restatement the kernels are tested against).
// Two streaming kernels: the fit (stack read once, diff + per-image min / max written) and blur + threshold (diff read
// once through an LDS tile with halo).  Algorithmic bytes per pixel: T sizeof(in) + 4 + 4 + 4.
#include "az_common.h"

#define TIR_TW 64  // output tile of the blur kernel: 64 x 32 pixels, 256 threads
#define TIR_TH 32
#define TIR_MAX_T 16
#define TIR_MAX_KS 31

// The (min, max) words of image i are mm[TIR_MM_STRIDE * i + 0 / 1]: one 256-byte line per image, so that the atomics
// of different images drain through different memory channels (az_common.h: ~4 ns per atomic on one channel).
#define TIR_MM_STRIDE 64
__global__ void tir_init_kernel(unsigned *mm, int B) {
    const int i = blockIdx.x * 64 + threadIdx.x;
    if (i < B) { mm[TIR_MM_STRIDE * i] = 0xffffffffu; mm[TIR_MM_STRIDE * i + 1] = 0u; }
}

// VEC consecutive grey levels of one exposure as floats; VEC = 4: one 16-byte (float) / 4-byte (uint8) load
template <int VEC> __device__ __forceinline__ void tir_load(const float *p, float (&v)[VEC]) {
    if constexpr (VEC == 4) {
        const float4 t = *reinterpret_cast<const float4 *>(p);
        v[0] = t.x; v[1] = t.y; v[2] = t.z; v[3] = t.w;
    } else {
        v[0] = p[0];
    }
}
template <int VEC> __device__ __forceinline__ void tir_load(const uint8_t *p, float (&v)[VEC]) {
    if constexpr (VEC == 4) {
        const unsigned t = *reinterpret_cast<const unsigned *>(p);
        v[0] = (float)(t & 255u); v[1] = (float)((t >> 8) & 255u); v[2] = (float)((t >> 16) & 255u); v[3] = (float)(t >> 24);
    } else {
        v[0] = (float)p[0];
    }
}

// One thread = VEC neighbouring pixels per step of a grid-stride walk over image blockIdx.y; every exposure is read as
// one coalesced row of the block.  sum (x - xbar)(y - ybar) = sum (x - xbar)(y - y[0]) because sum (x - xbar) = 0: one
// pass, no mean, and the differences keep the products small (exact in fp32 for integer grey levels: multiples of 1/2
// below 2^16).  The grid is capped (tir_fit_blocks) and a block folds its four waves' extrema in LDS before its ONE
// atomic pair: with an atomic pair per wave of a one-step grid, 32 400 atomics into one line at B = 8, 540 x 960, a call
// took 0.40 ms whatever the input type; this way 0.05 ms (profiles/temporal_ir_kernel_trace.md).
template <typename IN_T, int VEC>
__global__ void __launch_bounds__(256)
tir_fit_kernel(float *__restrict__ diff, unsigned *__restrict__ mm, const IN_T *__restrict__ stack, int T, int hw,
               float sxx) {
    __shared__ float wave_mn[4], wave_mx[4];
    const int img = blockIdx.y;
    const IN_T *base = stack + (size_t)img * T * hw;
    const float xbar = 0.5f * (float)(T - 1);
    float mn = 3.4e38f, mx = 0.f;
    // (VEC = 4 only with hw % 4 == 0: i < hw means i + 3 < hw as well)
    for (long long i = ((long long)blockIdx.x * 256 + threadIdx.x) * VEC; i < hw; i += (long long)gridDim.x * 256 * VEC) {
        const IN_T *p = base + i;
        float y0[VEC], num[VEC];
        tir_load<VEC>(p, y0);
#pragma unroll
        for (int v = 0; v < VEC; ++v) num[v] = 0.f;
#pragma unroll 4
        for (int t = 1; t < T; ++t) {
            float y[VEC];
            tir_load<VEC>(p + (size_t)t * hw, y);
            const float c = (float)t - xbar;
#pragma unroll
            for (int v = 0; v < VEC; ++v) num[v] += c * (y[v] - y0[v]);
        }
        float d[VEC];
#pragma unroll
        for (int v = 0; v < VEC; ++v) {
            d[v] = fabsf(num[v] / sxx * (float)(T - 1)) / 255.f;
            mn = fminf(mn, d[v]);
            mx = fmaxf(mx, d[v]);
        }
        float *q = diff + (size_t)img * hw + i;
        if constexpr (VEC == 4) {
            *reinterpret_cast<float4 *>(q) = make_float4(d[0], d[1], d[2], d[3]);
        } else {
            q[0] = d[0];
        }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        mn = fminf(mn, __shfl_xor(mn, o));
        mx = fmaxf(mx, __shfl_xor(mx, o));
    }
    if ((threadIdx.x & 63) == 0) { wave_mn[threadIdx.x >> 6] = mn; wave_mx[threadIdx.x >> 6] = mx; }
    __syncthreads();
    if (threadIdx.x == 0) {
        mn = fminf(fminf(wave_mn[0], wave_mn[1]), fminf(wave_mn[2], wave_mn[3]));
        mx = fmaxf(fmaxf(wave_mx[0], wave_mx[1]), fmaxf(wave_mx[2], wave_mx[3]));
        // non-negative floats order like their bit patterns
        if (mn <= mx) {
            atomicMin(&mm[TIR_MM_STRIDE * img], __float_as_uint(mn));
            atomicMax(&mm[TIR_MM_STRIDE * img + 1], __float_as_uint(mx));
        }
    }
}

// BORDER_REFLECT_101 for an index at most n - 1 outside [0, n)
__device__ __forceinline__ int tir_reflect(int i, int n) { return i < 0 ? -i : (i >= n ? 2 * (n - 1) - i : i); }

// One workgroup = one 64 x 32 output tile of image blockIdx.z.  LDS: the normalised tile with its halo of r = ks / 2,
// [TH + 2r][TW + 2r], then the row sums [TH + 2r][TW]; ks = 31: (62 * 94 + 62 * 64) * 4 = 39 184 bytes.
// Halo cells whose pixel lies more than r beyond the image (ragged tiles) feed no output of the image: they are not
// loaded -- reflecting them could leave the image -- and hold zero.
__global__ void __launch_bounds__(256)
tir_blur_threshold_kernel(float *__restrict__ out, const float *__restrict__ diff, const unsigned *__restrict__ mm,
                          int H, int W, int ks, float threshold) {
    extern __shared__ float tir_lds[];
    const int r = ks >> 1, SW = TIR_TW + 2 * r, SH = TIR_TH + 2 * r;
    float *st = tir_lds, *rs = tir_lds + SH * SW;
    const int img = blockIdx.z, x0 = blockIdx.x * TIR_TW, y0 = blockIdx.y * TIR_TH;
    const float mn = __uint_as_float(mm[TIR_MM_STRIDE * img]), mx = __uint_as_float(mm[TIR_MM_STRIDE * img + 1]);
    const float range = mx - mn, inv_sw = 1.f / (float)SW;
    const float *p = diff + (size_t)img * H * W;
    for (int i = threadIdx.x; i < SH * SW; i += 256) {
        const int ly = (int)(((float)i + 0.5f) * inv_sw), lx = i - ly * SW;  // = i / SW: i < 2^13, no quotient within 2^-8 of an integer
        const int gy = y0 - r + ly, gx = x0 - r + lx;
        float v = 0.f;
        if (gy < H + r && gx < W + r) v = (p[tir_reflect(gy, H) * W + tir_reflect(gx, W)] - mn) / range;
        st[i] = v;
    }
    __syncthreads();
    for (int i = threadIdx.x; i < SH * TIR_TW; i += 256) {  // row sums: lanes along x, conflict-free
        const float *s = st + (i >> 6) * SW + (i & 63);
        float a = 0.f;
        for (int k = 0; k < ks; ++k) a += s[k];
        rs[i] = a;
    }
    __syncthreads();
    const int x = threadIdx.x & 63, gx = x0 + x;
    const float area = (float)(ks * ks);
    for (int oy = threadIdx.x >> 6; oy < TIR_TH; oy += 4) {
        const int gy = y0 + oy;
        if (gy >= H || gx >= W) continue;
        float a = 0.f;
        for (int k = 0; k < ks; ++k) a += rs[(oy + k) * TIR_TW + x];
        const float d = st[(oy + r) * SW + x + r];
        // max == min: the reference normalises to NaN and every comparison is false -- all zeros
        out[(size_t)img * H * W + gy * W + gx] = (range > 0.f && d - a / area > threshold) ? 1.f : 0.f;
    }
}

static inline long long tir_diff_offset(int B) { return (long long)TIR_MM_STRIDE * B; }  // floats in front of the diff images
// blocks per image of the fit: every block of a one-step grid, at most about 2048 over the batch (8 per CU)
static inline int tir_fit_blocks(int hw, int vec, int B) {
    const int need = (hw / vec + 255) / 256, cap = 2048 / B > 64 ? 2048 / B : 64;
    return need < cap ? need : cap;
}

extern "C" long long az_temporal_ir_workspace(int B, int T, int H, int W, int ks) {
    if (B <= 0 || H <= 0 || W <= 0) return AZ_EINVAL;
    if (T < 2 || T > TIR_MAX_T) return AZ_EUNSUPPORTED;
    if (ks < 3 || ks > TIR_MAX_KS || (ks & 1) == 0) return AZ_EUNSUPPORTED;
    if (H <= ks / 2 || W <= ks / 2) return AZ_EINVAL;  // a single reflection must suffice
    if ((long long)H * W > 0x7fffffffLL || B > 65535) return AZ_EUNSUPPORTED;
    return (tir_diff_offset(B) + (long long)B * H * W) * 4;
}

template <typename IN_T>
static void tir_launch_fit(float *diff, unsigned *mm, const void *stack, bool vec, int B, int T, int hw, hipStream_t s) {
    const float sxx = (float)(T * (T * T - 1)) / 12.f;  // sum (x - xbar)^2, a multiple of 1/2
    const IN_T *in = static_cast<const IN_T *>(stack);
    if (vec)
        hipLaunchKernelGGL((tir_fit_kernel<IN_T, 4>), dim3(tir_fit_blocks(hw, 4, B), B), dim3(256), 0, s, diff, mm, in, T, hw, sxx);
    else
        hipLaunchKernelGGL((tir_fit_kernel<IN_T, 1>), dim3(tir_fit_blocks(hw, 1, B), B), dim3(256), 0, s, diff, mm, in, T, hw, sxx);
}

extern "C" int az_temporal_ir(float *pattern, float *workspace, long long workspace_bytes, const void *stack,
                              int stack_is_u8, int B, int T, int H, int W, int ks, float threshold, void *stream) {
    if (pattern == nullptr || workspace == nullptr || stack == nullptr) return AZ_EINVAL;
    const long long need = az_temporal_ir_workspace(B, T, H, W, ks);
    if (need < 0) return (int)need;
    if (workspace_bytes < need) return AZ_EWORKSPACE;
    hipStream_t s = az_stream(stream);
    unsigned *mm = reinterpret_cast<unsigned *>(workspace);
    float *diff = workspace + tir_diff_offset(B);
    const int hw = H * W;
    // four pixels per load where every exposure of every image starts on a vector boundary
    const bool vec = hw % 4 == 0 && (uintptr_t)diff % 16 == 0 && (uintptr_t)stack % (stack_is_u8 ? 4 : 16) == 0;
    hipLaunchKernelGGL(tir_init_kernel, dim3((B + 63) / 64), dim3(64), 0, s, mm, B);
    if (stack_is_u8)
        tir_launch_fit<uint8_t>(diff, mm, stack, vec, B, T, hw, s);
    else
        tir_launch_fit<float>(diff, mm, stack, vec, B, T, hw, s);
    const int r = ks / 2;
    const size_t lds = (size_t)(TIR_TH + 2 * r) * (2 * TIR_TW + 2 * r) * sizeof(float);
    hipLaunchKernelGGL(tir_blur_threshold_kernel, dim3((W + TIR_TW - 1) / TIR_TW, (H + TIR_TH - 1) / TIR_TH, B), dim3(256),
                       lds, s, pattern, diff, mm, H, W, ks, threshold);
    return az_launch_status();
}
