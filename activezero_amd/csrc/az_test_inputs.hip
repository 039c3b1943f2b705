// K25 and K26 -- the two per-pixel passes of a test item that the evaluation kernels (K18, K22, K23, K24) left on the host
// or to ATen (include/azhip.h has the rules).
//
// K25 az_depth_labels: reference datasets/messytable.py:197-213, 256-261, 281-284.  The loader divides two 1080 x 1920
// 16-bit millimetre maps by 1000 in float64, builds focal_length * baseline / depth under a mask in float64, casts four
// maps to float32 and uploads them: 33 MB per item.  Here the uint16 (or int32) maps are uploaded as they are, 8.3 MB, and
// one launch writes the four float32 maps with numpy's bits: the same two IEEE double divisions, each result rounded to
// float32 once.  The training crop 2x : 2(x + th) is a per-item window origin read on the device.
//
// K26 az_test_images: reference test.py:118-131, 141-146 -- two F.interpolate(mode="bilinear", align_corners=False) and two
// F.pad, four launches and four intermediates per item -- as one launch for both views: the output tensor, pad included, is
// written once.  The source is either the normalised 3-channel float image the reference's loader delivers (22 MB for a
// 720 x 1280 pair) or the 8-bit grey levels themselves (1.8 MB), normalised per channel at every tap with K20's bits.
//
// Both kernels: a thread owns four neighbouring columns of an output row, 16-byte stores when the row pitch is a multiple
// of four and the tensors are aligned (the entry points decide), one guarded 4-byte store per column otherwise; grid-stride
// over 64-bit indices.  Every float operation is rounded once: nothing below may contract into an fma.
#include "az_common.h"

#pragma clang fp contract(off)

#define TI_BLOCK 256

__device__ __forceinline__ void ti_store4(float *o, const float (&q)[4], int n, bool vec) {
    if (vec) {  // the pitch is a multiple of four: n == 4
        *reinterpret_cast<float4 *>(o) = make_float4(q[0], q[1], q[2], q[3]);
    } else {
#pragma unroll
        for (int j = 0; j < 4; ++j)
            if (j < n) o[j] = q[j];
    }
}

// ---- K25 -----------------------------------------------------------------------------------------------------------
// n (1..4) raw values from p; one 8-byte (uint16) or 16-byte (int32) load where the quad is whole and the address allows --
// it depends on the window origin, which only the device knows
template <class T>
__device__ __forceinline__ void dl_load4(const T *p, int n, int (&v)[4]) {
    if (n == 4 && (reinterpret_cast<uintptr_t>(p) & (4 * sizeof(T) - 1)) == 0) {
        if constexpr (sizeof(T) == 2) {
            const uint2 t = *reinterpret_cast<const uint2 *>(p);
            v[0] = (int)(t.x & 0xffffu); v[1] = (int)(t.x >> 16); v[2] = (int)(t.y & 0xffffu); v[3] = (int)(t.y >> 16);
        } else {
            const int4 t = *reinterpret_cast<const int4 *>(p);
            v[0] = t.x; v[1] = t.y; v[2] = t.z; v[3] = t.w;
        }
    } else {
#pragma unroll
        for (int j = 0; j < 4; ++j) v[j] = j < n ? (int)p[j] : 0;
    }
}

// numpy's lines: z = v / 1000 in double; disp = fb / z where z > 0 (v > 0), else 0; both rounded to float32 once
__device__ __forceinline__ void dl_labels(const int (&v)[4], double fb, float (&disp)[4], float (&depth)[4]) {
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const double z = (double)v[j] / 1000.0;
        depth[j] = (float)z;
        disp[j] = v[j] > 0 ? (float)(fb / z) : 0.0f;
    }
}

template <class T>
__global__ void __launch_bounds__(TI_BLOCK)
depth_labels_kernel(float *__restrict__ disp_l, float *__restrict__ depth_l, float *__restrict__ disp_r,
                    float *__restrict__ depth_r, const T *__restrict__ mm_l, const T *__restrict__ mm_r,
                    const double *__restrict__ focal_length, const double *__restrict__ baseline,
                    const int *__restrict__ origin, int H2, int W2, int h2, int w2, int quads_per_row, long long quads,
                    int vec_out) {
    for (long long i = (long long)blockIdx.x * TI_BLOCK + threadIdx.x; i < quads; i += (long long)gridDim.x * TI_BLOCK) {
        const long long row = i / quads_per_row;
        const int x = 4 * (int)(i - row * quads_per_row), b = (int)(row / h2), y = (int)(row - (long long)b * h2);
        int y0 = 0, x0 = 0;
        if (origin != nullptr) {  // a device-side value cannot be refused: it is clamped, the window never leaves the map
            y0 = min(max(origin[2 * b], 0), H2 - h2);
            x0 = min(max(origin[2 * b + 1], 0), W2 - w2);
        }
        const double fb = focal_length[b] * baseline[b];
        const size_t in = ((size_t)b * H2 + (size_t)(y0 + y)) * W2 + (size_t)(x0 + x);
        const size_t out = ((size_t)b * h2 + (size_t)y) * w2 + (size_t)x;
        const int n = min(4, w2 - x);
        int vl[4], vr[4];
        dl_load4(mm_l + in, n, vl);
        dl_load4(mm_r + in, n, vr);
        float disp[4], depth[4];
        dl_labels(vl, fb, disp, depth);
        ti_store4(disp_l + out, disp, n, vec_out);
        ti_store4(depth_l + out, depth, n, vec_out);
        dl_labels(vr, fb, disp, depth);
        ti_store4(disp_r + out, disp, n, vec_out);
        ti_store4(depth_r + out, depth, n, vec_out);
    }
}

static bool ti_aligned16(const void *p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

extern "C" int az_depth_labels(float *disp_l, float *depth_l, float *disp_r, float *depth_r, const void *mm_l,
                               const void *mm_r, int dtype, const double *focal_length, const double *baseline,
                               const int32_t *origin, int B, int H2, int W2, int h2, int w2, void *stream) {
    AZ_REQUIRE_PTR(disp_l); AZ_REQUIRE_PTR(depth_l); AZ_REQUIRE_PTR(disp_r); AZ_REQUIRE_PTR(depth_r);
    AZ_REQUIRE_PTR(mm_l); AZ_REQUIRE_PTR(mm_r); AZ_REQUIRE_PTR(focal_length); AZ_REQUIRE_PTR(baseline);
    AZ_REQUIRE(dtype == AZ_DEPTH_U16 || dtype == AZ_DEPTH_I32);
    AZ_REQUIRE(B > 0 && H2 > 0 && W2 > 0 && h2 > 0 && w2 > 0);
    AZ_REQUIRE(h2 <= H2 && w2 <= W2);                             // the window fits the map ...
    AZ_REQUIRE(origin != nullptr || (h2 == H2 && w2 == W2));      // ... and without an origin it is the map
    const int quads_per_row = (w2 - 1) / 4 + 1;
    if ((long long)B * h2 > 0x7fffffffffffLL / quads_per_row) return AZ_EUNSUPPORTED;
    const long long quads = (long long)B * h2 * quads_per_row;
    const int vec_out = w2 % 4 == 0 && ti_aligned16(disp_l) && ti_aligned16(depth_l) && ti_aligned16(disp_r) &&
                        ti_aligned16(depth_r);
    const dim3 grid(az_grid_for(quads, TI_BLOCK)), block(TI_BLOCK);
    hipStream_t s = az_stream(stream);
    if (dtype == AZ_DEPTH_U16)
        hipLaunchKernelGGL(depth_labels_kernel<uint16_t>, grid, block, 0, s, disp_l, depth_l, disp_r, depth_r,
                           static_cast<const uint16_t *>(mm_l), static_cast<const uint16_t *>(mm_r), focal_length, baseline,
                           origin, H2, W2, h2, w2, quads_per_row, quads, vec_out);
    else
        hipLaunchKernelGGL(depth_labels_kernel<int32_t>, grid, block, 0, s, disp_l, depth_l, disp_r, depth_r,
                           static_cast<const int32_t *>(mm_l), static_cast<const int32_t *>(mm_r), focal_length, baseline,
                           origin, H2, W2, h2, w2, quads_per_row, quads, vec_out);
    return az_launch_status();
}

// ---- K26 -----------------------------------------------------------------------------------------------------------
// ATen's upsample_bilinear2d source position for align_corners=False, in float32, each operation rounded on its own:
// src = max(scale (dst + 0.5) - 0.5, 0), i0 = (int)src, i1 = i0 + (i0 < in - 1), l1 = src - i0, l0 = 1 - l1
struct ti_axis {
    int i0, i1;
    float l0, l1;
};

__device__ __forceinline__ ti_axis ti_source(int dst, float scale, int in) {
    const float src = fmaxf(scale * ((float)dst + 0.5f) - 0.5f, 0.0f);
    ti_axis a;
    a.i0 = min((int)src, in - 1);  // (src < in - 0.5 for every dst < out: the min never acts, it only bounds the address)
    a.i1 = a.i0 + (a.i0 < in - 1 ? 1 : 0);
    a.l1 = src - (float)a.i0;
    a.l0 = 1.0f - a.l1;
    return a;
}

// Each product and sum of the blend is made opaque to the optimiser: left alone, hipcc packs the products of a pixel in
// pairs (v_pk_mul_f32) and adds the two halves of a pair with v_pk_add_f32 op_sel:[0,1] -- the high register selected for
// src1, the form that returns wrong values beside MFMA waves of another kernel (profiles/r03_pkfma_corun.md;
// tests/test_isa_lint_cpu.py keeps it out of the library).  The kernel waits for memory, not for these nine operations.
__device__ __forceinline__ float ti_alone(float v) {
    asm("" : "+v"(v));
    return v;
}

__device__ __forceinline__ float ti_blend(const ti_axis &ay, const ti_axis &ax, float a, float b, float c, float d) {
    const float top = ti_alone(ti_alone(ax.l0 * a) + ti_alone(ax.l1 * b));
    const float bottom = ti_alone(ti_alone(ax.l0 * c) + ti_alone(ax.l1 * d));
    return ti_alone(ti_alone(ay.l0 * top) + ti_alone(ay.l1 * bottom));
}

// U8: src [N,Hin,Win] grey levels, every tap normalised per channel; else src [N,3,Hin,Win] float32.  Images n >= n_first
// come from src_second (the right view): both views leave in one launch without being stacked first.
template <bool U8>
__global__ void __launch_bounds__(TI_BLOCK)
test_images_kernel(float *__restrict__ out, const void *__restrict__ src_first, const void *__restrict__ src_second,
                   int n_first, int Hin, int Win, int H, int W, int top_pad, int Hp, int Wp, float scale_h, float scale_w,
                   int quads_per_row, long long quads, int vec_out) {
    // the 256 levels of each channel, normalised once per workgroup with K20's operations: float32 v / 255, minus the
    // mean, divided by the std, every division correctly rounded -- the taps are then LDS reads, not 2 x 48 divisions
    __shared__ float level[U8 ? 768 : 1];
    if constexpr (U8) {
        const float mean[3] = {0.485f, 0.456f, 0.406f}, stdv[3] = {0.229f, 0.224f, 0.225f};
#pragma unroll
        for (int ch = 0; ch < 3; ++ch) level[256 * ch + threadIdx.x] = ((float)threadIdx.x / 255.f - mean[ch]) / stdv[ch];
        __syncthreads();
    }
    const size_t in_plane = (size_t)Hin * Win, out_plane = (size_t)Hp * Wp;
    for (long long i = (long long)blockIdx.x * TI_BLOCK + threadIdx.x; i < quads; i += (long long)gridDim.x * TI_BLOCK) {
        const long long row = i / quads_per_row;
        const int x = 4 * (int)(i - row * quads_per_row), n = (int)(row / Hp), yo = (int)(row - (long long)n * Hp);
        const int cols = min(4, Wp - x);
        float *o = out + ((size_t)n * 3 * Hp + (size_t)yo) * Wp + (size_t)x;
        float q[3][4];
#pragma unroll
        for (int ch = 0; ch < 3; ++ch)
#pragma unroll
            for (int j = 0; j < 4; ++j) q[ch][j] = 0.0f;  // the pad: +0.0
        if (yo >= top_pad && x < W) {
            const ti_axis ay = ti_source(yo - top_pad, scale_h, Hin);
            ti_axis ax[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) ax[j] = ti_source(min(x + j, W - 1), scale_w, Win);
            const int m = n < n_first ? n : n - n_first;
            const void *base = n < n_first ? src_first : src_second;
            const size_t r0 = (size_t)ay.i0 * Win, r1 = (size_t)ay.i1 * Win;
            if constexpr (U8) {
                const uint8_t *p = static_cast<const uint8_t *>(base) + (size_t)m * in_plane;
                int t[4][4];
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    t[j][0] = p[r0 + ax[j].i0]; t[j][1] = p[r0 + ax[j].i1];
                    t[j][2] = p[r1 + ax[j].i0]; t[j][3] = p[r1 + ax[j].i1];
                }
#pragma unroll
                for (int ch = 0; ch < 3; ++ch) {
                    const float *lv = level + 256 * ch;
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        const float v = ti_blend(ay, ax[j], lv[t[j][0]], lv[t[j][1]], lv[t[j][2]], lv[t[j][3]]);
                        q[ch][j] = x + j < W ? v : 0.0f;  // selected, never multiplied: a NaN tap stays out of the pad
                    }
                }
            } else {
#pragma unroll
                for (int ch = 0; ch < 3; ++ch) {
                    const float *p = static_cast<const float *>(base) + ((size_t)m * 3 + ch) * in_plane;
                    float t[4][4];
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        t[j][0] = p[r0 + ax[j].i0]; t[j][1] = p[r0 + ax[j].i1];
                        t[j][2] = p[r1 + ax[j].i0]; t[j][3] = p[r1 + ax[j].i1];
                    }
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        const float v = ti_blend(ay, ax[j], t[j][0], t[j][1], t[j][2], t[j][3]);
                        q[ch][j] = x + j < W ? v : 0.0f;
                    }
                }
            }
        }
#pragma unroll
        for (int ch = 0; ch < 3; ++ch) ti_store4(o + ch * out_plane, q[ch], cols, vec_out);
    }
}

extern "C" int az_test_images(float *out, const void *src, const void *src_second, int src_is_u8, int N, int N_second,
                              int Hin, int Win, int H, int W, int top_pad, int right_pad, void *stream) {
    AZ_REQUIRE_PTR(out); AZ_REQUIRE_PTR(src);
    if (N_second > 0) AZ_REQUIRE_PTR(src_second);
    AZ_REQUIRE(src_is_u8 == 0 || src_is_u8 == 1);
    AZ_REQUIRE(N > 0 && N_second >= 0 && Hin > 0 && Win > 0 && H > 0 && W > 0 && top_pad >= 0 && right_pad >= 0);
    const long long Hp = (long long)H + top_pad, Wp = (long long)W + right_pad, images = (long long)N + N_second;
    if (Hp > 0x7fffffffLL || Wp > 0x7fffffffLL - 3 || images > 0x7fffffffLL) return AZ_EUNSUPPORTED;
    const int quads_per_row = (int)((Wp + 3) / 4);
    if (images * Hp > 0x7fffffffffffLL / quads_per_row) return AZ_EUNSUPPORTED;
    const long long quads = images * Hp * quads_per_row;
    const int vec_out = Wp % 4 == 0 && ti_aligned16(out);
    // ATen's scale when a size is given: (float)in / out
    const float scale_h = (float)Hin / (float)H, scale_w = (float)Win / (float)W;
    const dim3 grid(az_grid_for(quads, TI_BLOCK)), block(TI_BLOCK);
    hipStream_t s = az_stream(stream);
    if (src_is_u8)
        hipLaunchKernelGGL(test_images_kernel<true>, grid, block, 0, s, out, src, src_second, N, Hin, Win, H, W, top_pad,
                           (int)Hp, (int)Wp, scale_h, scale_w, quads_per_row, quads, vec_out);
    else
        hipLaunchKernelGGL(test_images_kernel<false>, grid, block, 0, s, out, src, src_second, N, Hin, Win, H, W, top_pad,
                           (int)Hp, (int)Wp, scale_h, scale_w, quads_per_row, quads, vec_out);
    return az_launch_status();
}
