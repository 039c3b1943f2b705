// Shared by the gather convolution kernels (az_conv3d.hip, az_conv3d_m128.hip, az_conv3d_t2.hip, az_conv2d.hip): one wave
// holds 32x32 MFMA accumulator tiles of an output patch -- lane & 31 = output channel, registers = voxels -- and these are
// the pieces that do not depend on how a kernel got there: the finish of one output element, the BatchNorm moments of a
// wave's tiles, and the commit / fragment read of the 24-dword slab image.  The block -> tile map, the C-layout row map and
// the slab image's offsets are index arithmetic: az_launch_math.h (swept on the CPU).
#pragma once
#include "az_roll_common.h"
#include "az_launch_math.h"

// EPI 0 of the 3-D kernels, one element: y = acc * scale + shift (+ residual) (ReLU), stored at out[off]
__device__ __forceinline__ void az_store_affine(float *outp, const float *resp, unsigned off, float acc, float sc, float sf,
                                                int relu) {
    float y = acc * sc + sf;
    if (resp) y += resp[off];
    if (relu) y = az_relu(y);
    outp[off] = y;
}

// BatchNorm moments of one channel over MT accumulator tiles of a wave: get(m, r) = register r of tile m in this lane, bit
// (m * 16 + r) of okmask = that voxel lies inside the output, nvalid = their number in this lane (FULL: every voxel does, no
// masking).  The two half-waves hold the two halves of a channel's voxels and are merged; s = the sum, m2 = the sum of
// squares about the tile's own mean (az_bn3d_finalize merges tiles by Chan's formula), returned: the voxel count.
template <int MT, bool FULL, class GET>
__device__ __forceinline__ int az_tile_moments(unsigned okmask, int nvalid, GET get, float &s, float &m2) {
    const int ntot = nvalid + __shfl_xor(nvalid, 32);
    s = 0.f;
    m2 = 0.f;
#pragma unroll
    for (int m = 0; m < MT; ++m)
#pragma unroll
        for (int r = 0; r < 16; ++r) s += (FULL || ((okmask >> (m * 16 + r)) & 1u)) ? get(m, r) : 0.f;
    s += __shfl_xor(s, 32);
    const float mean = s / (float)(FULL ? MT * 32 : max(ntot, 1));
#pragma unroll
    for (int m = 0; m < MT; ++m)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const float dlt = get(m, r) - mean;
            m2 += (FULL || ((okmask >> (m * 16 + r)) & 1u)) ? dlt * dlt : 0.f;
        }
    m2 += __shfl_xor(m2, 32);
    return ntot;
}
// ... stored under the canonical tile id: part[channel][tile] = (s, m2) by the lower half-wave, cnt[tile] by channel 0's lane
__device__ __forceinline__ void az_tile_moments_store(float *part, float *cnt, long long ntiles, int co, int tile_id, int half,
                                                      float s, float m2, int ntot) {
    if (half == 0) {
        *reinterpret_cast<float2 *>(&part[((size_t)co * ntiles + tile_id) * 2]) = make_float2(s, m2);
        if (co == 0) cnt[tile_id] = (float)ntot;
    }
}

// ---- the 24-dword slab image (az_launch_math.h: az_s24_write_off / az_s24_read_base) -----------------------------------
// AR, the arithmetic: 0 = bf16x6 (three bf16 parts), 1 = f16x3 (two fp16 parts of v * in_scale), 2 = one bf16 part,
// 3 = one fp16 part of v * in_scale
// commit of one staged float4 = channels 4j .. 4j + 3 of voxel (sy, sx)
template <int AR>
__device__ __forceinline__ void az_s24_commit(unsigned *slab, int sy, int sx, int j, int pitch, const float4 &v, float in_scale) {
    unsigned *dst = slab + az_s24_write_off(sy, sx, j, pitch);
    if constexpr (AR == 0) {
        uint2 hi, mid, lo;
        az_split3_bf16x4(v, hi, mid, lo);
        *reinterpret_cast<uint2 *>(dst) = hi;
        *reinterpret_cast<uint2 *>(dst + 8) = mid;
        *reinterpret_cast<uint2 *>(dst + 16) = lo;
    } else if constexpr (AR == 1) {
        uint2 hi, lo;
        az_split2_f16x4(make_float4(v.x * in_scale, v.y * in_scale, v.z * in_scale, v.w * in_scale), hi, lo);
        *reinterpret_cast<uint2 *>(dst) = hi;
        *reinterpret_cast<uint2 *>(dst + 8) = lo;
    } else if constexpr (AR == 2) {
        *reinterpret_cast<uint2 *>(dst) = make_uint2(az_pk_bf16(v.x, v.y), az_pk_bf16(v.z, v.w));
    } else {
        *reinterpret_cast<uint2 *>(dst) = make_uint2(az_pk_f16(v.x * in_scale, v.y * in_scale), az_pk_f16(v.z * in_scale, v.w * in_scale));
    }
}
// The A fragments: a lane keeps two bases (az_s24_read_base; the parity of the tap row decides the half swap), everything else
// is a wave-uniform offset of the ds_read.  ap: base + that offset; the NP parts' fragments of the voxel there.
template <int NP>
__device__ __forceinline__ void az_s24_load(float4 (&aq)[3], const float *ap) {
#pragma unroll
    for (int p = 0; p < NP; ++p) aq[p] = *reinterpret_cast<const float4 *>(ap + 8 * p);
}
