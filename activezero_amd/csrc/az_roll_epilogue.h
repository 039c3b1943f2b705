// The two pieces every rolling convolution kernel ends with (az_conv3d_roll.hip, az_conv2d_roll.hip, az_conv3d_s2roll.hip,
// az_conv3d_t2roll.hip), stated once: the output epilogue y = relu?(acc * scale + shift (+ residual)) of one 16-byte piece,
// and the BatchNorm partials of the raw-output launches (EPI 1).  Everything about a kernel's geometry -- which voxel a lane
// owns, offsets, validity masks, the tile ids of its partial rows -- stays in the kernel.
#pragma once
#include "az_roll_common.h"

typedef __amdgpu_buffer_rsrc_t az_rsrc;

// ---- BatchNorm partials (EPI 1) ----------------------------------------------------------------------------------------------
// ONE entry (n * mean, M2) per channel, and one count, for everything a wave produces over its whole walk (a 4x16 half patch
// over a depth segment, a patch quarter over the images of a group, ...).  Every lane keeps running sums of the values it
// owns about a shift of its own (the first valid value it sees: shifted-data algorithm, no cancellation in sum-of-squares
// minus squared-sum) -- a subtract, an add and an FMA per value and no cross-lane traffic; the lanes of a channel are merged
// once, after the walk (Chan's formula).  The first version of az_conv3d_roll.hip reduced every plane to a (sum, centred M2)
// entry of its own (~100 VALU and four cross-lane sums per plane, 9 spilled registers, 97 920 partial rows per V0 layer for the
// finalize kernels to merge; this form: no spills, 4 080 rows, no pre-merge launch).  Both cost nothing measurable in the
// kernel itself: 1.42 ms with or without statistics (profiles/r03_roll_kernel_notes.md section 6 -- the 0.2 ms "epilogue gap"
// quoted earlier was the timing script measuring this kernel first, before the clocks had settled).
template <int N>
struct RollSums {  // of N channels in one lane: shifts k, sums of (v - k), sums of (v - k)^2
    // (three arrays, not an array of triples: the other layout moves hipcc's register allocation in the kernels that sit at
    //  the 256-register limit -- as does the order in which the four updates of a voxel are written, hence add_voxel AND add)
    float k[N], s1[N], s2[N];
    __device__ __forceinline__ RollSums() {
#pragma unroll
        for (int i = 0; i < N; ++i) { k[i] = 0.f; s1[i] = 0.f; s2[i] = 0.f; }
    }
    // k[i]: the kernel sets it, before the first update, to the first valid value this lane meets (any value near the data
    // serves); when a lane meets it differs from kernel to kernel, so the assignment stays there
    __device__ __forceinline__ void add(int i, float v, bool ok) {
        const float d = ok ? v - k[i] : 0.f;
        s1[i] += d;
        s2[i] = fmaf(d, d, s2[i]);
    }
    // channel-per-lane accumulators: the four elements of tile v belong to channel i; element r is valid iff e0 + r < nv
    __device__ __forceinline__ void add_tile(int i, const f32x4 &v, int e0, int nv) {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const float d = (e0 + r < nv) ? v[r] - k[i] : 0.f;
            s1[i] += d;
            s2[i] = fmaf(d, d, s2[i]);
        }
    }
    // voxel-per-lane accumulators: y holds one voxel's values of the channels i0 .. i0 + 3 (az_conv3d_roll.hip calls add()
    // four times instead: differences first, as here, costs its 64-channel statistics kernels 6 to 7 more spilled registers)
    __device__ __forceinline__ void add_voxel(int i0, const float4 &y, bool ok) {
        const float d0 = ok ? y.x - k[i0] : 0.f, d1 = ok ? y.y - k[i0 + 1] : 0.f, d2 = ok ? y.z - k[i0 + 2] : 0.f, d3 = ok ? y.w - k[i0 + 3] : 0.f;
        s1[i0] += d0; s1[i0 + 1] += d1; s1[i0 + 2] += d2; s1[i0 + 3] += d3;
        s2[i0] = fmaf(d0, d0, s2[i0]); s2[i0 + 1] = fmaf(d1, d1, s2[i0 + 1]);
        s2[i0 + 2] = fmaf(d2, d2, s2[i0 + 2]); s2[i0 + 3] = fmaf(d3, d3, s2[i0 + 3]);
    }
};

// Chan's merge over the lanes lane ^ off, off = LO, 2 LO, .. < HI: <16, 64> where a lane is a channel and the four 16-lane
// row groups share it (r16_step / r16_step3 accumulators), <1, 16> where a lane is a voxel and its 16-lane group shares four
// channels (r16_chain9 / R_MH accumulators).  Every lane of the group ends with the group's (n, mean, M2).
template <int LO, int HI>
__device__ __forceinline__ void az_roll_merge_lanes(float &n, float &mean, float &m2) {
#pragma unroll
    for (int off = LO; off < HI; off <<= 1) {
        const float n_o = __shfl_xor(n, off), mean_o = __shfl_xor(mean, off), m2_o = __shfl_xor(m2, off);
        const float nn = n + n_o;
        const float dlt = mean_o - mean;
        const float w_o = nn > 0.f ? n_o / nn : 0.f;
        m2 = m2 + m2_o + dlt * dlt * n * w_o;
        mean = mean + dlt * w_o;
        n = nn;
    }
}

// after the walk: the lane group's entry (n * mean, max(M2, 0)) of one channel from every lane's sums (k, s1, s2) over its n
// values, written at byte offset `off` of the partial buffer (R_OOB in the lanes that do not write); returns the group's count
template <int LO, int HI>
__device__ __forceinline__ float az_roll_flush_channel(const float &k, const float &s1, const float &s2, float n, az_rsrc rs_part, unsigned off) {
    float mean = n > 0.f ? k + s1 / n : 0.f;  // mean and centred second moment of this lane's values (0 for none)
    float m2 = n > 0.f ? s2 - s1 * s1 / n : 0.f;
    az_roll_merge_lanes<LO, HI>(n, mean, m2);
    __builtin_amdgcn_raw_buffer_store_b64(__builtin_bit_cast(u32x2, make_float2(n * mean, fmaxf(m2, 0.f))), rs_part, off, 0, 0);
    return n;
}

// ---- output epilogue ---------------------------------------------------------------------------------------------------------
// scale / shift of the lane's four consecutive channels c .. c + 3 (1 / 0 where there is none, or for load = false)
__device__ __forceinline__ void az_roll_load_affine(bool load, const float *scale, const float *shift, int c, float4 &sc, float4 &sf) {
    sc = make_float4(1.f, 1.f, 1.f, 1.f); sf = make_float4(0.f, 0.f, 0.f, 0.f);
    if (load) {
        if (scale) sc = *reinterpret_cast<const float4 *>(scale + c);
        if (shift) sf = *reinterpret_cast<const float4 *>(shift + c);
    }
}
// f16x3: the power-of-two unscaling rides on the affine map (e beyond the float range: the true result is, too)
__device__ __forceinline__ void az_roll_ldexp4(float4 &sc, int e) {
    sc.x = ldexpf(sc.x, e); sc.y = ldexpf(sc.y, e); sc.z = ldexpf(sc.z, e); sc.w = ldexpf(sc.w, e);
}

// acc * scale + shift in the two forms the kernels were written and measured in: a product and a sum that the compiler may
// contract (the channel-per-lane kernels), and an explicit FMA (the voxel-per-lane kernels).  They are not interchangeable
// bit for bit wherever the compiler does not contract: each kernel keeps its own.
__device__ __forceinline__ float4 az_roll_affine_mul(const f32x4 v, const float4 sc, const float4 sf) {
    return make_float4(v[0] * sc.x + sf.x, v[1] * sc.y + sf.y, v[2] * sc.z + sf.z, v[3] * sc.w + sf.w);
}
__device__ __forceinline__ float4 az_roll_affine_fma(const f32x4 v, const float4 sc, const float4 sf) {
    return make_float4(fmaf(v[0], sc.x, sf.x), fmaf(v[1], sc.y, sf.y), fmaf(v[2], sc.z, sf.z), fmaf(v[3], sc.w, sf.w));
}

// the finish of one 16-byte piece: + residual (RES; read at roff), floor (FLOOR: 0 for a ReLU, -inf for none; a NaN stays NaN
// under either, az_max_nan), store at off;
// offsets are R_OOB in the lanes whose voxel is outside.  Returns what it stored.
template <bool RES, bool FLOOR>
__device__ __forceinline__ float4 az_roll_finish_piece(float4 y, az_rsrc rs_res, unsigned roff, float floor_, az_rsrc rs_out, unsigned off) {
    if (RES) {
        const float4 rr = __builtin_bit_cast(float4, __builtin_amdgcn_raw_buffer_load_b128(rs_res, roff, 0, 0));
        y.x += rr.x; y.y += rr.y; y.z += rr.z; y.w += rr.w;
    }
    if (FLOOR) { y.x = az_max_nan(y.x, floor_); y.y = az_max_nan(y.y, floor_); y.z = az_max_nan(y.z, floor_); y.w = az_max_nan(y.w, floor_); }
    __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4, y), rs_out, off, 0, 0);
    return y;
}
