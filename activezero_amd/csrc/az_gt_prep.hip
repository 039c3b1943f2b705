// K18 -- the sim step's ground truth from the right view in one launch: reference train.py:255-272 (test.py:91-110 with
// fixed sizes), the chain
//     F.interpolate(disp_R / depth, mode="nearest")  ->  .type(torch.int)  ->  apply_disparity_cu (sign check with two host
//     syncs, zero-filled result, scatter kernel)  ->  (disp < hi) * (disp > lo)
// The structure is az_warp_scatter.hip's: one 64-lane wavefront owns one output row (n, y) for all channels;
//   pass 1  winner[t] = min { j : j + trunc(d[j]) == t } by LDS integer atomicMin -- order independent, deterministic;
//   pass 2  coalesced stores of disp_l / extra_l (winner's value or 0), keep_s (resized only) and the mask byte.
// The row is read straight from the full-resolution maps at ATen's legacy "nearest" source indices
// min((int)floorf(dst * scale), in - 1): no resized intermediate, no int tensor.  For the factor 0.5 the loads are
// stride-2 dwords of every other row: half of each fetched 64-byte line is used, a quarter of the source is touched at all.
// Pass 2 reads the winner's disparity again (the same lines, L1 / L2 hits) instead of holding a second row in LDS.
// Each pass issues the loads of four lane passes together (GTP_U).
// Counters: a wave sums its lanes (popcount of a ballot), a workgroup its four waves in LDS, then ONE global atomicAdd
// per counter and workgroup, issued only when non-zero (540 workgroups at B = 4, 540 x 960).
#include "az_common.h"

#define GTP_U 4  // lane passes whose loads are issued together

// ATen's legacy nearest source index; the float clamp keeps the conversion defined for any finite scale
__device__ __forceinline__ int gtp_src(int dst, float scale, int in) {
    const int i = (int)fminf(floorf((float)dst * scale), 2.0e9f);
    return i < in - 1 ? i : in - 1;
}

__global__ void __launch_bounds__(256)
gt_from_right_kernel(float *__restrict__ disp_l, float *__restrict__ extra_l, float *__restrict__ keep_s,
                     uint8_t *__restrict__ mask, int *__restrict__ stats, const float *__restrict__ disp_r,
                     const float *__restrict__ extra, const float *__restrict__ keep, int Ce, int Ck, int Hin, int Win,
                     int H, int W, float scale_h, float scale_w, float lo, float hi, int rows) {
    extern __shared__ int gtp_winner_all[];
    __shared__ int wave_bad[4], wave_cnt[4];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    int *winner = gtp_winner_all + wave * W;
    const int row = blockIdx.x * 4 + wave;  // (n, y)
    const bool active = row < rows;         // idle waves of the last workgroup still reach every barrier
    const int none = 0x7fffffff;
    const int n = active ? row / H : 0, y = active ? row - n * H : 0;
    const int ys = gtp_src(y, scale_h, Hin);
    const size_t in_plane = (size_t)Hin * Win, out_plane = (size_t)H * W;
    const float *drow = disp_r + (size_t)n * in_plane + (size_t)ys * Win;
    int bad = 0, cnt = 0;
    for (int t = lane; t < W; t += 64) winner[t] = none;
    __syncthreads();
    // Both passes walk the row GTP_U lane passes at a time and issue that chunk's loads together (columns past the end
    // are clamped to the last one: always a valid address, the value is dropped): a wave has only W / 64 dependent
    // steps and the grid only ~8 waves per CU at 540 x 960, so the loads in flight per wave set the rate.
    if (active) {
        for (int j0 = lane; j0 < W; j0 += 64 * GTP_U) {
            float d[GTP_U];
#pragma unroll
            for (int u = 0; u < GTP_U; ++u) d[u] = drow[gtp_src(min(j0 + 64 * u, W - 1), scale_w, Win)];
#pragma unroll
            for (int u = 0; u < GTP_U; ++u) {
                const int j = j0 + 64 * u;
                if (j >= W) continue;
                // compared as a float BEFORE the conversion: NaN, +-inf and d <= -1 are counted and land nowhere
                // (the reference's sign assertion); d >= W lands nowhere; d in (-1, 0) truncates to 0
                if (!(d[u] > -1.0f) || d[u] == __builtin_inff()) {
                    ++bad;
                } else if (d[u] < (float)W) {
                    const int t = j + (int)d[u];
                    if (t < W) atomicMin(&winner[t], j);
                }
            }
        }
    }
    __syncthreads();
    if (active) {
        const size_t out_row = (size_t)y * W, in_row = (size_t)ys * Win;
        float *dl = disp_l + (size_t)n * out_plane + out_row;
        uint8_t *mk = mask != nullptr ? mask + (size_t)n * out_plane + out_row : nullptr;
        for (int t0 = lane; t0 < W + lane; t0 += 64 * GTP_U) {  // (every lane makes the same number of trips: the ballot)
            int xj[GTP_U], xt[GTP_U];
            bool hit[GTP_U];
            float v[GTP_U];
#pragma unroll
            for (int u = 0; u < GTP_U; ++u) {
                const int t = min(t0 + 64 * u, W - 1), j = winner[t];
                hit[u] = j != none;
                xj[u] = gtp_src(hit[u] ? j : 0, scale_w, Win);
                xt[u] = gtp_src(t, scale_w, Win);
            }
#pragma unroll
            for (int u = 0; u < GTP_U; ++u) v[u] = drow[xj[u]];
#pragma unroll
            for (int u = 0; u < GTP_U; ++u) {
                const int t = t0 + 64 * u;
                v[u] = hit[u] ? v[u] : 0.0f;
                const bool on = t < W && lo < v[u] && v[u] < hi;
                if (t < W) {
                    dl[t] = v[u];
                    if (mk != nullptr) mk[t] = on ? 1 : 0;
                }
                cnt += __popcll(__ballot(on));  // wave-uniform
            }
            for (int c = 0; c < Ce; ++c) {
                const float *er = extra + ((size_t)n * Ce + c) * in_plane + in_row;
                float *eo = extra_l + ((size_t)n * Ce + c) * out_plane + out_row;
                float e[GTP_U];
#pragma unroll
                for (int u = 0; u < GTP_U; ++u) e[u] = er[xj[u]];
#pragma unroll
                for (int u = 0; u < GTP_U; ++u)
                    if (t0 + 64 * u < W) eo[t0 + 64 * u] = hit[u] ? e[u] : 0.0f;
            }
            for (int c = 0; c < Ck; ++c) {
                const float *kr = keep + ((size_t)n * Ck + c) * in_plane + in_row;
                float *ko = keep_s + ((size_t)n * Ck + c) * out_plane + out_row;
                float k[GTP_U];
#pragma unroll
                for (int u = 0; u < GTP_U; ++u) k[u] = kr[xt[u]];
#pragma unroll
                for (int u = 0; u < GTP_U; ++u)
                    if (t0 + 64 * u < W) ko[t0 + 64 * u] = k[u];
            }
        }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) bad += __shfl_xor(bad, o);
    if (lane == 0) { wave_bad[wave] = bad; wave_cnt[wave] = cnt; }
    __syncthreads();
    if (threadIdx.x == 0) {
        const int b = wave_bad[0] + wave_bad[1] + wave_bad[2] + wave_bad[3];
        const int c = wave_cnt[0] + wave_cnt[1] + wave_cnt[2] + wave_cnt[3];
        if (b != 0) atomicAdd(&stats[0], b);
        if (c != 0) atomicAdd(&stats[1], c);
    }
}

extern "C" int az_gt_from_right(float *disp_l, float *extra_l, float *keep_s, uint8_t *mask, int32_t *stats,
                                const float *disp_r, const float *extra, const float *keep, int N, int Ce, int Ck,
                                int Hin, int Win, int H, int W, float scale_h, float scale_w, float lo, float hi,
                                void *stream) {
    if (disp_l == nullptr || stats == nullptr || disp_r == nullptr) return AZ_EINVAL;
    if (Ce < 0 || Ck < 0) return AZ_EINVAL;
    if ((Ce > 0) != (extra != nullptr) || (Ce > 0) != (extra_l != nullptr)) return AZ_EINVAL;
    if ((Ck > 0) != (keep != nullptr) || (Ck > 0) != (keep_s != nullptr)) return AZ_EINVAL;
    AZ_REQUIRE(N > 0 && Hin > 0 && Win > 0 && H > 0 && W > 0);
    AZ_REQUIRE(scale_h > 0.0f && scale_w > 0.0f && scale_h < __builtin_inff() && scale_w < __builtin_inff());
    if (H > Hin || W > Win) return AZ_EUNSUPPORTED;                        // no upsampling
    // W <= 4096, the limit of az_warp_scatter: the four winner rows then fill 64 KiB of dynamic LDS; with the 32 bytes of
    // static counters the workgroup asks for 65 568 bytes, inside the 160 KiB a gfx950 workgroup may have
    if ((size_t)W * 4 * sizeof(int) > 64 * 1024) return AZ_EUNSUPPORTED;
    if ((long long)N * H > 0x7fffffffLL / 4) return AZ_EUNSUPPORTED;
    const int rows = N * H;
    const unsigned grid = (rows + 3) / 4;
    const size_t lds = (size_t)W * 4 * sizeof(int);
    hipLaunchKernelGGL(gt_from_right_kernel, dim3(grid), dim3(256), lds, az_stream(stream), disp_l, extra_l, keep_s, mask,
                       stats, disp_r, extra, keep, Ce, Ck, Hin, Win, H, W, scale_h, scale_w, lo, hi, rows);
    return az_launch_status();
}
