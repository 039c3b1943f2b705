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

// K23 -- the evaluation mask of a test instance in one launch: reference test.py:112-117, 162-193, the chain
//     F.interpolate(robot_mask, mode="nearest").type(torch.int) == 0,  F.interpolate(realsense_depth, mode="nearest") > 0,
//     (disp < max_disp) * (disp > 0) * ((depth > 0) & (depth < 1.25)) * robot * realsense  ->  .type(torch.bool)
// One thread per output pixel: the auxiliary maps are read at gtp_src's indices in their OWN type (the loader delivers
// float64; a float32 round trip could turn 0.99999999 into 1 before the truncating cast), no resized, integer or boolean
// intermediate exists.  The count: popcount of a ballot per wave, LDS over the workgroup's waves, one atomic per
// workgroup, issued only when non-zero.
struct em_aux {  // an optional auxiliary map [B,h,w]
    const void *p;
    int f64, h, w;
    float scale_h, scale_w;
};

template <class T>
__device__ __forceinline__ T em_read(const em_aux &a, int b, int y, int x) {
    const int ys = gtp_src(y, a.scale_h, a.h), xs = gtp_src(x, a.scale_w, a.w);
    return static_cast<const T *>(a.p)[((size_t)b * a.h + ys) * a.w + xs];
}

__global__ void __launch_bounds__(256)
eval_mask_kernel(uint8_t *__restrict__ mask, int *__restrict__ count, const float *__restrict__ disp_l,
                 const float *__restrict__ depth_l, em_aux robot, em_aux rs, int H, int W, long long n, float max_disp,
                 int exclude_bg, float depth_hi) {
    __shared__ int wave_cnt[4];
    int cnt = 0;
    // (every lane of a wave makes the same trips: the ballot)
    for (long long i0 = (long long)blockIdx.x * 256 + (threadIdx.x & ~63); i0 < n; i0 += (long long)gridDim.x * 256) {
        const long long i = i0 + (threadIdx.x & 63);
        bool on = false;
        if (i < n) {
            const float d = disp_l[i];
            on = 0.f < d && d < max_disp;
            if (exclude_bg) {
                const float z = depth_l[i];
                on = on && 0.f < z && z < depth_hi;
            }
            const long long row = i / W;
            const int x = (int)(i - row * W), b = (int)(row / H), y = (int)(row - (long long)b * H);
            if (robot.p != nullptr)  // (int) truncates toward zero, as .type(torch.int) does
                on = on && (robot.f64 ? (int)em_read<double>(robot, b, y, x) : (int)em_read<float>(robot, b, y, x)) == 0;
            if (rs.p != nullptr) on = on && (rs.f64 ? em_read<double>(rs, b, y, x) > 0.0 : em_read<float>(rs, b, y, x) > 0.f);
            mask[i] = on ? 1 : 0;
        }
        cnt += __popcll(__ballot(on));  // wave-uniform
    }
    if ((threadIdx.x & 63) == 0) wave_cnt[threadIdx.x >> 6] = cnt;
    __syncthreads();
    if (threadIdx.x == 0) {
        const int c = wave_cnt[0] + wave_cnt[1] + wave_cnt[2] + wave_cnt[3];
        if (c != 0) atomicAdd(count, c);
    }
}

static bool em_aux_ok(const void *p, int f64, int h, int w) {
    return (f64 == 0 || f64 == 1) && (p == nullptr || (h > 0 && w > 0));
}

extern "C" int az_eval_mask(uint8_t *mask, int32_t *count, const float *disp_l, const float *depth_l, const void *robot,
                            int robot_f64, int Hr, int Wr, const void *realsense, int realsense_f64, int Hs, int Ws, int B,
                            int H, int W, float max_disp, int exclude_bg, float depth_hi, void *stream) {
    AZ_REQUIRE_PTR(mask); AZ_REQUIRE_PTR(count); AZ_REQUIRE_PTR(disp_l);
    if (exclude_bg) AZ_REQUIRE_PTR(depth_l);
    AZ_REQUIRE(B > 0 && H > 0 && W > 0);
    AZ_REQUIRE(em_aux_ok(robot, robot_f64, Hr, Wr) && em_aux_ok(realsense, realsense_f64, Hs, Ws));
    // ATen's scale when a size is given: (float)in / out
    const em_aux a_robot = {robot, robot_f64, Hr, Wr, (float)Hr / (float)H, (float)Wr / (float)W};
    const em_aux a_rs = {realsense, realsense_f64, Hs, Ws, (float)Hs / (float)H, (float)Ws / (float)W};
    const long long n = (long long)B * H * W;
    hipStream_t s = az_stream(stream);
    if (hipMemsetAsync(count, 0, sizeof(int32_t), s) != hipSuccess) return AZ_ELAUNCH;  // (the zeroing is included)
    hipLaunchKernelGGL(eval_mask_kernel, dim3(az_grid_for(n, 256)), dim3(256), 0, s, mask, count, disp_l, depth_l, a_robot,
                       a_rs, H, W, n, max_disp, exclude_bg, depth_hi);
    return az_launch_status();
}
