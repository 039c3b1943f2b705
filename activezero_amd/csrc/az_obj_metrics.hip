// K22 -- the error metrics of a test batch per image and per object label in ONE pass: reference
// utils/cascade_metrics.py:65-126 compute_obj_err (label.unique().tolist() -- a host sync --, then per object a
// (label == obj) & mask temporary and a chain of masked reductions over the whole map) and, with no label map, the
// per-image form of compute_err_metric.  A pixel is read once (four float maps, the mask byte, the label: 21 B, 17 B
// without labels); its terms (az_disp_terms.h, shared with K12) go to the counters of (image, label).
//
// Shape.  A workgroup lies inside one image: OM_BLOCK threads stride over that image's pixels, so focal_x_baseline[b]
// and the accumulator rows acc[b] are uniform per workgroup.  Its counters live in LDS ([L] rows of two fp64 sums and
// seven integers).  What reaches them is already summed over the lanes that share a label:
//   * fast path -- every live lane of the wave holds the same in-range label (labels are spatially coherent: nearly
//     always): lanes keep adding to their own registers, as K12's do, for as long as that label lasts; the registers
//     are summed over the wave (shuffles) and added to the LDS row by one lane per counter only when the wave's label
//     changes and at the end.
//   * mixed wave -- one round per distinct label: the counts are popcounts of ballots, the two sums shuffle trees over
//     the label's lanes (the others add 0), then one lane per counter adds to LDS.  64 labels in a wave cost 64 rounds;
//     that is the price of a case the data does not have, not of the common one.
// So an LDS counter sees at most one add per wave and label run, never 64 same-address adds from one wave
// (az_block_reduce.h records what same-address serialisation cost K12).  At the end a workgroup issues ONE global atomic
// per (label it met, slot) whose value is not zero -- lanes e = 8 l + slot, i.e. contiguous 8-byte addresses -- one per
// label for `present`, and one for stats.  No per-pixel global atomic exists.  The grid is capped at OM_GRID_CAP
// workgroups over ALL images (4 per CU; max(1, 1024 / B) per image), so at most 1024 / B adds meet on one address.  The
// flush is what the cap is for: with 1024 workgroups PER image (B = 4, 540 x 960: 4096 workgroups, two trips per wave
// instead of eight) the kernel took 48.0 us with 17 labels and 53.8 us with none, against 35.5 us and 23.8 us under
// this cap -- the same-address adds cost more than the shorter loop saves (tools/bench_aux_kernels.py eval_epilogue).
// Counts are exact integers (an image has fewer than 2^31 pixels); the order of the fp64 sums is unspecified, as in K12.
#include "az_common.h"
#include "az_disp_terms.h"

#define OM_BLOCK 256
#define OM_GRID_CAP 1024  // workgroups over all images
#define OM_NCNT 7         // integer counters per label: five thresholds, the masked count, presence

// which accumulator slot an integer counter belongs to (presence has a row of its own)
__device__ __forceinline__ constexpr int om_slot_of(int c) {
    return c == 0 ? AZ_DM_BAD1 : c == 1 ? AZ_DM_BAD2 : c == 2 ? AZ_DM_Z2 : c == 3 ? AZ_DM_Z4 : c == 4 ? AZ_DM_Z8 : AZ_DM_COUNT;
}

__device__ __forceinline__ double om_wave_sum(double x) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) x += __shfl_xor(x, off);
    return x;
}
__device__ __forceinline__ int om_wave_sum(int x) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) x += __shfl_xor(x, off);
    return x;
}

// wave totals (the same in every lane) -> the LDS row of label l: one lane per counter, nothing for a zero
__device__ __forceinline__ void om_to_lds(double (*s_sum)[2], int (*s_cnt)[OM_NCNT], int l, int lane, double epe, double mm,
                                          const int (&c)[OM_NCNT]) {
    int mine = 0;
#pragma unroll
    for (int k = 0; k < OM_NCNT; ++k) mine = lane == k ? c[k] : mine;
    if (lane < OM_NCNT && mine != 0) atomicAdd(&s_cnt[l][lane], mine);
    if (lane == OM_NCNT && epe != 0.0) atomicAdd(&s_sum[l][0], epe);
    if (lane == OM_NCNT + 1 && mm != 0.0) atomicAdd(&s_sum[l][1], mm);
}

__global__ void __launch_bounds__(OM_BLOCK)
obj_metrics_kernel(double *__restrict__ acc, int *__restrict__ present, int *__restrict__ stats,
                   const float *__restrict__ disp_gt, const float *__restrict__ depth_gt,
                   const float *__restrict__ disp_pred, const float *__restrict__ depth_pred,
                   const float *__restrict__ fb, const unsigned char *__restrict__ mask, const int *__restrict__ label,
                   int L, long long per_image, int blocks_per_image) {
    __shared__ double s_sum[AZ_OBJ_MAX_LABELS][2];
    __shared__ int s_cnt[AZ_OBJ_MAX_LABELS][OM_NCNT];
    __shared__ int s_bad;
    const int lane = threadIdx.x & 63;
    const int b = blockIdx.x / blocks_per_image, j = blockIdx.x - b * blocks_per_image;
    for (int e = threadIdx.x; e < L * OM_NCNT; e += OM_BLOCK) (&s_cnt[0][0])[e] = 0;
    for (int e = threadIdx.x; e < L * 2; e += OM_BLOCK) (&s_sum[0][0])[e] = 0.0;
    if (threadIdx.x == 0) s_bad = 0;
    __syncthreads();

    const size_t img = (size_t)b * (size_t)per_image;
    const float fbv = depth_pred ? 0.f : fb[b];
    const long long stride = (long long)blocks_per_image * OM_BLOCK;
    int cur = -1;  // the label the lane registers below belong to (wave-uniform), -1: none
    double r_epe = 0.0, r_mm = 0.0;
    int r_c[OM_NCNT] = {0, 0, 0, 0, 0, 0, 0};
    int bad = 0;
    // i0: the wave's first pixel of this trip (wave-uniform: every lane of a wave makes the same trips)
    for (long long i0 = (long long)j * OM_BLOCK + (threadIdx.x & ~63); i0 < per_image; i0 += stride) {
        const bool live = i0 + lane < per_image;
        const size_t i = img + (size_t)(live ? i0 + lane : per_image - 1);  // a dead lane reads a valid address, drops the value
        const int lb_raw = label ? label[i] : 0;
        const bool on = live && mask[i] != 0;
        const float dp = disp_pred[i];
        const float zp = depth_pred ? depth_pred[i] : az_dm_depth(fbv, dp);
        const az_dm_px p = az_dm_pixel(disp_gt[i], depth_gt[i], dp, zp);
        const bool in_range = (unsigned)lb_raw < (unsigned)L;
        bad += live && !in_range ? 1 : 0;
        const int lb = live && in_range ? lb_raw : -1;  // -1: takes part in nothing below
        const int c[OM_NCNT] = {on && p.bad1, on && p.bad2, on && p.z2, on && p.z4, on && p.z8, on, lb >= 0};
        // a masked-off pixel adds 0, never its own value times 0: its NaN must not reach the sums
        const float t_epe = on ? p.dd : 0.f, t_mm = on ? p.dmm : 0.f;

        const unsigned long long members = __ballot(lb >= 0);
        if (members == 0) continue;
        const int first = __shfl(lb, __ffsll((long long)members) - 1);
        if (__ballot(lb == first) == __ballot(live)) {  // one label in the whole wave
            if (first != cur) {
                if (cur >= 0) {
                    int w[OM_NCNT];
#pragma unroll
                    for (int k = 0; k < OM_NCNT; ++k) { w[k] = om_wave_sum(r_c[k]); r_c[k] = 0; }
                    om_to_lds(s_sum, s_cnt, cur, lane, om_wave_sum(r_epe), om_wave_sum(r_mm), w);
                    r_epe = r_mm = 0.0;
                }
                cur = first;
            }
            r_epe += (double)t_epe;
            r_mm += (double)t_mm;
#pragma unroll
            for (int k = 0; k < OM_NCNT; ++k) r_c[k] += c[k];
            continue;
        }
        unsigned long long todo = members;
        while (todo != 0) {  // one round per distinct label of the wave
            const int l = __shfl(lb, __ffsll((long long)todo) - 1);
            const bool mine = lb == l;
            todo &= ~__ballot(mine);
            int w[OM_NCNT];
#pragma unroll
            for (int k = 0; k < OM_NCNT; ++k) w[k] = __popcll(__ballot(mine && c[k] != 0));
            double epe = 0.0, mm = 0.0;
            if (w[OM_NCNT - 2] != 0) {  // some masked pixel of this label: only then can a sum be non-zero
                epe = om_wave_sum(mine ? (double)t_epe : 0.0);
                mm = om_wave_sum(mine ? (double)t_mm : 0.0);
            }
            om_to_lds(s_sum, s_cnt, l, lane, epe, mm, w);
        }
    }
    if (cur >= 0) {
        int w[OM_NCNT];
#pragma unroll
        for (int k = 0; k < OM_NCNT; ++k) w[k] = om_wave_sum(r_c[k]);
        om_to_lds(s_sum, s_cnt, cur, lane, om_wave_sum(r_epe), om_wave_sum(r_mm), w);
    }
    bad = om_wave_sum(bad);
    if (lane == 0 && bad != 0) atomicAdd(&s_bad, bad);
    __syncthreads();

    // the flush: lanes e = 8 l + slot are contiguous 8-byte addresses of acc[b]; a zero is not sent
    double *row = acc + (size_t)b * L * AZ_DM_SLOTS;
    for (int e = threadIdx.x; e < L * AZ_DM_SLOTS; e += OM_BLOCK) {
        const int l = e / AZ_DM_SLOTS, slot = e - l * AZ_DM_SLOTS;
        double x = slot == AZ_DM_EPE ? s_sum[l][0] : slot == AZ_DM_MM ? s_sum[l][1] : 0.0;
#pragma unroll
        for (int k = 0; k < OM_NCNT - 1; ++k)
            if (slot == om_slot_of(k)) x = (double)s_cnt[l][k];
        if (x != 0.0) atomicAdd(&row[e], x);  // (a NaN is not zero: it is sent)
    }
    for (int l = threadIdx.x; l < L; l += OM_BLOCK)
        if (s_cnt[l][OM_NCNT - 1] != 0) atomicAdd(&present[(size_t)b * L + l], s_cnt[l][OM_NCNT - 1]);
    if (threadIdx.x == 0 && s_bad != 0) atomicAdd(&stats[0], s_bad);
}

extern "C" int az_obj_metrics(double *acc, int32_t *present, int32_t *stats, const float *disp_gt, const float *depth_gt,
                              const float *disp_pred, const float *depth_pred, const float *focal_x_baseline,
                              const uint8_t *mask, const int32_t *label, int B, int L, long long per_image, void *stream) {
    AZ_REQUIRE_PTR(acc); AZ_REQUIRE_PTR(present); AZ_REQUIRE_PTR(stats);
    AZ_REQUIRE_PTR(disp_gt); AZ_REQUIRE_PTR(depth_gt); AZ_REQUIRE_PTR(disp_pred); AZ_REQUIRE_PTR(mask);
    if (!depth_pred) AZ_REQUIRE_PTR(focal_x_baseline);
    AZ_REQUIRE(B >= 0 && per_image >= 0 && L >= 1);
    if (L > AZ_OBJ_MAX_LABELS) return AZ_EUNSUPPORTED;
    if (per_image > 0x7fffffffLL) return AZ_EUNSUPPORTED;  // present[] and the counters are int32
    if (B == 0 || per_image == 0) return AZ_OK;
    long long bpi = (per_image + OM_BLOCK - 1) / OM_BLOCK;
    const long long cap = B >= OM_GRID_CAP ? 1 : OM_GRID_CAP / B;
    if (bpi > cap) bpi = cap;
    hipLaunchKernelGGL(obj_metrics_kernel, dim3((unsigned)(bpi * B)), dim3(OM_BLOCK), 0, az_stream(stream), acc, present,
                       stats, disp_gt, depth_gt, disp_pred, depth_pred, focal_x_baseline, mask, label, L, per_image,
                       (int)bpi);
    return az_launch_status();
}
