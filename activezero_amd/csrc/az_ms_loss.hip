// K29 -- the multi-scale masked smooth-L1 disparity loss: N predictions, prediction k at scale 2^-shift_k, against ONE
// full-resolution ground truth and mask (reference utils/losses.py:17-32 dispnet_disp: seven scales, and :71-72
// default_disp: one prediction at full resolution).  The reference resizes ground truth and mask to every scale with
// F.interpolate(scale_factor = 1 / 2^s) (nearest: destination (y, x) reads source (y << s, x << s), size (H >> s, W >> s)),
// compacts both operands with boolean indexing (a device->host sync each) and takes one smooth_l1 mean per scale; here
// every scale reads the full-resolution maps at the strided index, the mask is applied in registers and the sums of all
// predictions land in one fp64 accumulator vector -- one launch forward, one backward, no sync.
// HBM-bound: 4 B per prediction pixel read (and written in backward) plus the ground-truth lines the strided read touches;
// a few hundred kilobytes in all -- the point is the removed launches and syncs.
#include "az_block_reduce.h"
#include "az_common.h"
#include "az_smooth_l1.h"

// Launch layout.  Prediction k owns a contiguous run of workgroups; a workgroup strides over ITS prediction's B h_k w_k
// pixels in steps of (workgroups of k) * MS_BLOCK and decomposes the flat index into (b, y, x) for the strided read.
#define MS_BLOCK 256
#define MS_GRID_CAP 1024  // workgroups per prediction at most, forward and backward (4 per CU, as K12's reductions)

// the descriptors of one call, by value in the kernel arguments: no table upload, no sync
struct MsArgs {
    const float *pred[AZ_MS_LOSS_MAX];
    float *grad[AZ_MS_LOSS_MAX];
    long long n[AZ_MS_LOSS_MAX];      // B * h * w
    int first[AZ_MS_LOSS_MAX + 1];    // first workgroup of prediction k; first[nd] = the grid
    int shift[AZ_MS_LOSS_MAX], h[AZ_MS_LOSS_MAX], w[AZ_MS_LOSS_MAX];
    float weight[AZ_MS_LOSS_MAX];
    int nd;
};

// K12's dl_valid at the strided source pixel: mask byte != 0, or lo < gt < hi (a NaN gt is invalid)
__device__ __forceinline__ bool ms_valid(const unsigned char *mask, float gt, float lo, float hi, long long src) {
    return mask ? (mask[src] != 0) : (gt > lo && gt < hi);
}

// the prediction this workgroup belongs to (block-uniform)
__device__ __forceinline__ int ms_pred_of_block(const MsArgs &a) {
    int k = 0;
#pragma unroll
    for (int j = 1; j < AZ_MS_LOSS_MAX; ++j)
        if (j < a.nd && (int)blockIdx.x >= a.first[j]) k = j;
    return k;
}

// flat index i of a [B,1,h,w] prediction -> flat index of [B,1,H,W] pixel (y << shift, x << shift)
__device__ __forceinline__ long long ms_src(long long i, int shift, long long hw, int w, long long HW, int W) {
    if (shift == 0) return i;  // h == H, w == W
    const long long b = i / hw, r = i - b * hw;
    const long long y = r / w, x = r - y * w;
    return b * HW + (y << shift) * W + (x << shift);
}

// acc[2k] += sum of smooth_l1(pred_k - gt) over prediction k's valid pixels, acc[2k+1] += their count
__global__ void __launch_bounds__(MS_BLOCK)
ms_loss_fwd_kernel(double *__restrict__ acc, const MsArgs a, const float *__restrict__ gt,
                   const unsigned char *__restrict__ mask, float lo, float hi, long long HW, int W) {
    const int k = ms_pred_of_block(a);
    const float *__restrict__ p = a.pred[k];
    const int shift = a.shift[k], w = a.w[k];
    const long long hw = (long long)a.h[k] * w, n = a.n[k];
    const long long stride = (long long)(a.first[k + 1] - a.first[k]) * MS_BLOCK;
    double v[2] = {0.0, 0.0};
    for (long long i = (long long)((int)blockIdx.x - a.first[k]) * MS_BLOCK + threadIdx.x; i < n; i += stride) {
        const long long src = ms_src(i, shift, hw, w, HW, W);
        const float g = gt[src];
        if (!ms_valid(mask, g, lo, hi, src)) continue;
        const float d = fabsf(p[i] - g);
        v[0] += d < 1.f ? 0.5f * d * d : d - 0.5f;  // F.smooth_l1_loss, beta = 1 (as K12 writes it)
        v[1] += 1.0;
    }
    az_block_sum_f64<2, MS_BLOCK>(v, acc + 2 * k);
}

// d loss / d pred_k = w_k * gloss / count_k * clamp(pred_k - gt, -1, 1) on valid pixels, 0 elsewhere (selected, never
// multiplied: an empty scale has s = inf).  Predictions without a gradient pointer own no workgroup.
__global__ void __launch_bounds__(MS_BLOCK)
ms_loss_bwd_kernel(const MsArgs a, const float *__restrict__ gt, const unsigned char *__restrict__ mask, float lo,
                   float hi, const float *__restrict__ gloss, const double *__restrict__ acc, long long HW, int W) {
    const int k = ms_pred_of_block(a);
    const float *__restrict__ p = a.pred[k];
    float *__restrict__ gp = a.grad[k];
    const int shift = a.shift[k], w = a.w[k];
    const long long hw = (long long)a.h[k] * w, n = a.n[k];
    const long long stride = (long long)(a.first[k + 1] - a.first[k]) * MS_BLOCK;
    const float wk = a.weight[k];
    const float s = gloss[0] / (float)acc[2 * k + 1];
    for (long long i = (long long)((int)blockIdx.x - a.first[k]) * MS_BLOCK + threadIdx.x; i < n; i += stride) {
        const long long src = ms_src(i, shift, hw, w, HW, W);
        const float g = gt[src];
        const bool ok = ms_valid(mask, g, lo, hi, src);
        gp[i] = ok ? wk * s * dl_clamp1(p[i] - g) : 0.f;
    }
}

// validates the descriptors and lays the workgroups out; *grid = 0: nothing to launch
static int ms_fill(MsArgs &a, unsigned *grid, const AzMsLossDesc *descs, const float *weights, int nd, int B, int H, int W,
                   bool backward) {
    AZ_REQUIRE_PTR(descs);
    AZ_REQUIRE(nd >= 1 && nd <= AZ_MS_LOSS_MAX);
    AZ_REQUIRE(B >= 0 && H >= 0 && W >= 0);
    a = MsArgs{};
    a.nd = nd;
    long long blocks = 0;
    for (int k = 0; k < nd; ++k) {
        const AzMsLossDesc &d = descs[k];
        AZ_REQUIRE_PTR(d.pred);
        AZ_REQUIRE(d.shift >= 0 && d.shift <= 30);
        AZ_REQUIRE(d.h >= 1 && d.w >= 1 && d.h == (H >> d.shift) && d.w == (W >> d.shift));
        a.pred[k] = d.pred;
        a.grad[k] = backward ? d.grad : nullptr;
        a.shift[k] = d.shift, a.h[k] = d.h, a.w[k] = d.w;
        a.weight[k] = weights ? weights[k] : 1.f;
        a.n[k] = (long long)B * d.h * d.w;
        a.first[k] = (int)blocks;
        if (backward && !d.grad) continue;  // no gradient wanted: no workgroup, nothing written
        long long g = (a.n[k] + MS_BLOCK - 1) / MS_BLOCK;
        blocks += g > MS_GRID_CAP ? MS_GRID_CAP : g;
    }
    for (int k = nd; k <= AZ_MS_LOSS_MAX; ++k) a.first[k] = (int)blocks;
    *grid = (unsigned)blocks;
    return AZ_OK;
}

extern "C" int az_ms_loss_fwd(double *acc, const AzMsLossDesc *descs, int nd, const float *gt,
                              const unsigned char *mask, float lo, float hi, int B, int H, int W, void *stream) {
    AZ_REQUIRE_PTR(acc); AZ_REQUIRE_PTR(gt);
    MsArgs a;
    unsigned grid = 0;
    const int rc = ms_fill(a, &grid, descs, nullptr, nd, B, H, W, false);
    if (rc != AZ_OK) return rc;
    if (grid == 0) return AZ_OK;
    hipLaunchKernelGGL(ms_loss_fwd_kernel, dim3(grid), dim3(MS_BLOCK), 0, az_stream(stream), acc, a, gt, mask, lo, hi,
                       (long long)H * W, W);
    return az_launch_status();
}

extern "C" int az_ms_loss_bwd(const AzMsLossDesc *descs, const float *weights, int nd, const float *gt,
                              const unsigned char *mask, float lo, float hi, const float *gloss, const double *acc,
                              int B, int H, int W, void *stream) {
    AZ_REQUIRE_PTR(acc); AZ_REQUIRE_PTR(gt); AZ_REQUIRE_PTR(gloss); AZ_REQUIRE_PTR(weights);
    MsArgs a;
    unsigned grid = 0;
    const int rc = ms_fill(a, &grid, descs, weights, nd, B, H, W, true);
    if (rc != AZ_OK) return rc;
    if (grid == 0) return AZ_OK;
    hipLaunchKernelGGL(ms_loss_bwd_kernel, dim3(grid), dim3(MS_BLOCK), 0, az_stream(stream), a, gt, mask, lo, hi, gloss,
                       acc, (long long)H * W, W);
    return az_launch_status();
}
