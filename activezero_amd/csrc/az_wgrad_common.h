// Shared by the weight-gradient kernels (az_conv3d_wgrad.hip, az_conv3d_wgrad16.hip, az_conv3d_wgrad16s2.hip,
// az_conv2d_wgrad.hip, az_conv2d_wgrad16.hip): the transposing fragment read, the staging split of the f16x3 arithmetic
// (its operand scales: az_f16_scales, az_roll_common.h), the accumulate chains of both MFMA shapes, the tap-major atomic
// flush, and the launchers the files call across each other.  The lane geometry and C-layout maps are index arithmetic: az_launch_math.h (swept on the CPU).
#pragma once
#include <type_traits>

#include "az_roll_common.h"
#include "az_launch_math.h"

typedef short s16x4 __attribute__((ext_vector_type(4)));
typedef short s16x8 __attribute__((ext_vector_type(8)));
typedef s16x4 __attribute__((address_space(3))) * lds_s16x4_ptr;

// AR, the arithmetic of a kernel: 0 = bf16x6 (three bf16 parts, six MFMAs per K block), 1 = f16x3 (two scaled fp16 parts,
// three MFMAs; az_roll_common.h), 2 = one bf16 part, 3 = one scaled fp16 part (one MFMA: az_conv2d_wgrad.hip)
constexpr int az_wgrad_parts(int AR) { return AR == 0 ? 3 : AR == 1 ? 2 : 1; }

// One operand fragment (ds_read_b64_tr_b16 on a [k][32 ch] 16-bit image): k rows 0..3 at lo, 4..7 at hi.  Per 16-lane group,
// lane 4q + p gives the address of row q, columns 4p..4p+3, and lane i receives column i of the four rows: eight consecutive
// K values of the lane's channel.  The caller names the format (__builtin_bit_cast to az_bf16x8 / az_f16x8).
__device__ __forceinline__ s16x8 az_tr16_frag(const void *lo, const void *hi) {
    const s16x4 lo4 = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4_ptr)(lo));
    const s16x4 hi4 = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4_ptr)(hi));
    s16x8 v;
    v[0] = lo4[0]; v[1] = lo4[1]; v[2] = lo4[2]; v[3] = lo4[3];
    v[4] = hi4[0]; v[5] = hi4[1]; v[6] = hi4[2]; v[7] = hi4[3];
    return v;
}

// one MFMA of either shape (by accumulator type) and format; FR: az_bf16x8 or az_f16x8, whichever the kernel keeps
template <bool F16, class FR>
__device__ __forceinline__ f32x4 az_wgrad_mfma(const FR &a, const FR &b, const f32x4 &c) {
    if constexpr (F16) return __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(az_f16x8, a), __builtin_bit_cast(az_f16x8, b), c, 0, 0, 0);
    else return __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(az_bf16x8, a), __builtin_bit_cast(az_bf16x8, b), c, 0, 0, 0);
}
template <bool F16, class FR>
__device__ __forceinline__ az_f32x16 az_wgrad_mfma(const FR &a, const FR &b, const az_f32x16 &c) {
    if constexpr (F16) return __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(az_f16x8, a), __builtin_bit_cast(az_f16x8, b), c, 0, 0, 0);
    else return __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(az_bf16x8, a), __builtin_bit_cast(az_bf16x8, b), c, 0, 0, 0);
}
// One K block chained into the RUNNING accumulator, smallest terms first: bf16x6  a2 b0, a0 b2, a1 b1, a1 b0, a0 b1, a0 b0;
// f16x3  lo hi, hi lo, hi hi.  a / b: the parts' fragments, hi first.
template <int AR, class ACC, class FR>
__device__ __forceinline__ void az_wgrad_chain(ACC &acc, const FR *a, const FR *b) {
    constexpr bool F16 = AR == 1 || AR == 3;
    ACC c = acc;
    if constexpr (AR == 0) {
        c = az_wgrad_mfma<F16>(a[2], b[0], c);
        c = az_wgrad_mfma<F16>(a[0], b[2], c);
        c = az_wgrad_mfma<F16>(a[1], b[1], c);
    }
    if constexpr (AR <= 1) {
        c = az_wgrad_mfma<F16>(a[1], b[0], c);
        c = az_wgrad_mfma<F16>(a[0], b[1], c);
    }
    acc = az_wgrad_mfma<F16>(a[0], b[0], c);
}
// f16x3, four M blocks against one fine fragment: four independent chains, issued term by term
__device__ __forceinline__ void az_wgrad_chain4_f16x3(f32x4 (&acc)[4], const az_f16x8 (&a)[4][2], const az_f16x8 (&b)[2]) {
#pragma unroll
    for (int mb = 0; mb < 4; ++mb) acc[mb] = az_wgrad_mfma<true>(a[mb][1], b[0], acc[mb]);
#pragma unroll
    for (int mb = 0; mb < 4; ++mb) acc[mb] = az_wgrad_mfma<true>(a[mb][0], b[1], acc[mb]);
#pragma unroll
    for (int mb = 0; mb < 4; ++mb) acc[mb] = az_wgrad_mfma<true>(a[mb][0], b[0], acc[mb]);
}

// One staged 16-byte piece (four channels) -> the 8-byte pieces of its parts (`scale`: the fp16 arithmetics).
template <int AR>
__device__ __forceinline__ void az_wgrad_split(const float4 &v, float scale, uint2 &hi, uint2 &mid, uint2 &lo) {
    if constexpr (AR == 0) {
        az_split3_bf16x4(v, hi, mid, lo);
    } else if constexpr (AR == 1) {
        az_stage_f16x4<false>(__builtin_bit_cast(u32x4, v), scale, hi, mid);
        lo = mid;
    } else {
        hi = AR == 2 ? make_uint2(az_pk_bf16(v.x, v.y), az_pk_bf16(v.z, v.w))
                     : make_uint2(az_pk_f16(v.x * scale, v.y * scale), az_pk_f16(v.z * scale, v.w * scale));
        mid = lo = hi;
    }
}
// ... of a piece as the buffer loads of the r16 kernels return it; PS: the tensor is pre-split (f16x3 only)
template <int AR, bool PS = false>
__device__ __forceinline__ void az_wgrad_split(const u32x4 &raw, float scale, uint2 &hi, uint2 &mid, uint2 &lo) {
    if constexpr (AR == 1) {
        az_stage_f16x4<PS>(raw, scale, hi, mid);
        lo = mid;
    } else {
        az_wgrad_split<AR>(__builtin_bit_cast(float4, raw), scale, hi, mid, lo);
    }
}
// ... written part_stride elements of *dst apart (the LDS images keep their three-part strides in every arithmetic)
template <int AR, class T>
__device__ __forceinline__ void az_wgrad_store_parts(T *dst, unsigned part_stride, const uint2 &hi, const uint2 &mid, const uint2 &lo) {
    *reinterpret_cast<uint2 *>(dst) = hi;
    if (az_wgrad_parts(AR) >= 2) *reinterpret_cast<uint2 *>(dst + part_stride) = mid;
    if (az_wgrad_parts(AR) >= 3) *reinterpret_cast<uint2 *>(dst + 2 * part_stride) = lo;
}

// The flush of a 16x16 C block: a wave adds it into tap `tap` of the tap-major workspace ws[tap][CM][CN] with float atomics, rows
// (coarse channels) from m0, columns (fine channels) from n0; SCALE: times o_scale (the fp16 arithmetics).  acc by value and the
// kernel's own `lane`: by reference, or with the lane recomputed, the 2-D kernels allocate other registers.  The kernels at
// the register limit (the two 3-D r16 kernels) and the 32x32 kernels (the one-kd kernels, az_conv2d_wgrad.hip) keep this loop
// written out with the same maps: called as a function it moves their registers and spills.
template <bool SCALE>
__device__ __forceinline__ void az_wgrad_flush16(float *ws, int tap, int m0, int n0, int CM, int CN, f32x4 acc, float o_scale, int lane) {
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int m = m0 + az_mfma16_c_row(lane, r);
        atomicAdd(&ws[((size_t)tap * CM + m) * CN + n0 + az_mfma16_c_col(lane)], SCALE ? acc[r] * o_scale : acc[r]);
    }
}

// ---- host ---------------------------------------------------------------------------------------------------------------
// all 27 taps per wave on 16x16x32 tiles, four waves sharing one staged set (az_conv3d_wgrad16.hip)
int az_conv3d_wgrad_r16_launch(float *ws, const float *coarse, const float *fine, int B, int cm, int cn, int D, int H, int W, hipStream_t s,
                               const float *coarse_amax = nullptr, const float *fine_amax = nullptr, int split_mask = 0);
// stride 2, f16x3: eight waves sharing one staged set (az_conv3d_wgrad16s2.hip)
int az_conv3d_wgrad_s2r16_launch(float *ws, const float *coarse, const float *fine, int B, int cm, int cn, int Dc, int Hc, int Wc,
                                 int Df, int Hf, int Wf, hipStream_t s, const float *coarse_amax, const float *fine_amax, int split_mask);
// the 3x3 d1 2-D layers with 32 / 64 channels on either side (az_conv2d_wgrad16.hip)
int az_conv2d_wgrad_r16_launch(float *ws, const float *coarse, const float *fine, int B, int H, int W, int cm, int cn,
                               int cs_c, int cs_f, hipStream_t s, const float *coarse_amax, const float *fine_amax);
// tap-major workspace [27][cm][cn] -> PyTorch's [cm][cn][27] (az_conv3d_wgrad.hip)
int az_wgrad_unpack_launch(float *grad_w, const float *ws, int cm, int cn, hipStream_t s);

// split_mask (bit 0: the coarse, bit 1: the fine operand is pre-split) -> template argument: launch(integral_constant<int, mask>)
// for 0 <= split_mask <= MAX; false: no such instantiation
template <int MAX, class F>
inline bool az_wgrad_split_dispatch(int split_mask, F &&launch) {
    if (split_mask < 0 || split_mask > MAX) return false;
    if (split_mask == 0) launch(std::integral_constant<int, 0>{});
    else if (split_mask == 1) launch(std::integral_constant<int, 1>{});
    else if (split_mask == 2) launch(std::integral_constant<int, 2>{});
    else if constexpr (MAX >= 3) launch(std::integral_constant<int, 3>{});
    return true;
}
