// K24 -- the six result images of a test batch as finished RGBA bytes: reference test.py:208-209, 235-260 with
// utils/test_util.py:59-107 save_img, which copy four full-size float maps to the host, set [ground_mask] = -1, wrap them in
// np.ma.masked_where(x == -1, x) and send each through matplotlib's Normalize and viridis table inside plt.imsave, and the two
// error images of utils/util.py:143-244 (K19) through the same call -- six device-to-host copies and six matplotlib passes per
// instance, at batch size 1 only.  Here the [B][6][H][W][4] bytes are a per-pixel function of maps that are on the device:
// panels 0 pred_disp, 1 gt_disp, 2 disparity error, 3 pred_depth, 4 gt_depth, 5 depth error (include/azhip.h has the rules).
//
// Two launches.  matplotlib paints an unmasked NaN red only when the image has NO masked pixel (np.ma.is_masked(X) false: the
// bad mask is then isnan); with any masked pixel NaN goes through astype(int) and take(mode="clip") to table[0].  So
// result_flags_kernel first ORs into flags[b] bit m when panel m of image b has a bad pixel (a workgroup lies inside one
// image; shuffles over the wave, LDS over the waves, one atomic per workgroup and only when non-zero), and
// result_img_kernel reads the word.  13 B read per pixel in either kernel, 24 B written by the second.
//
// The render kernel: a thread owns four neighbouring pixels of a row, so a panel's 16 bytes leave as one store -- when
// W % 4 == 0 and the maps are aligned (the entry point decides; 540 x 960 tensors are); otherwise one pixel per thread and
// 4-byte accesses.  The 256-entry table sits in LDS (the lookups are random per lane); grid-stride over 64-bit indices.
//
// Every float operation below is rounded once: hipcc contracts a * s - b * s into an fma by default, which moves the depth
// error of panel 5 across a table row (the reference multiplies by 1000 in torch before its call, test.py:260).
#include "az_error_table.h"
#include "az_viridis_table.h"

#pragma clang fp contract(off)

#define RI_BLOCK 256
#define RI_FLAGS_GRID_CAP 1024  // workgroups of the reduce kernel over all images
#define RI_RED 0xff0000ffu      // R, G, B, A = 255, 0, 0, 255 in memory order
#define RI_BLACK 0xff000000u
#define RI_VIRIDIS_PANELS 0x1bu  // panels 0, 1, 3, 4

__device__ __forceinline__ const float *ri_pred_row(const float *pred, long long row_stride, long long img_stride, int b,
                                                    int y) {
    return pred + (long long)b * img_stride + (long long)y * row_stride;
}

__global__ void __launch_bounds__(RI_BLOCK)
result_flags_kernel(int *__restrict__ flags, const float *__restrict__ pred, long long pred_row_stride,
                    long long pred_img_stride, const float *__restrict__ gt_disp, const float *__restrict__ gt_depth,
                    const uint8_t *__restrict__ mask, const float *__restrict__ fb, int H, int W, int blocks_per_image) {
    __shared__ int wave_bits[RI_BLOCK / AZ_WAVE];
    const int b = blockIdx.x / blocks_per_image, j = blockIdx.x - b * blocks_per_image;
    const long long hw = (long long)H * W;
    const size_t img = (size_t)b * (size_t)hw;
    const float fbv = fb[b];
    int bits = 0;
    for (long long p = (long long)j * RI_BLOCK + threadIdx.x; p < hw; p += (long long)blocks_per_image * RI_BLOCK) {
        const int y = (int)(p / W), x = (int)(p - (long long)y * W);
        if (mask[img + p] == 0) {
            bits |= RI_VIRIDIS_PANELS;  // v = -1 in all four
        } else {
            const float pd = ri_pred_row(pred, pred_row_stride, pred_img_stride, b, y)[x];
            bits |= (pd == -1.0f ? 1 : 0) | (gt_disp[img + p] == -1.0f ? 2 : 0) | (fbv / pd == -1.0f ? 8 : 0) |
                    (gt_depth[img + p] == -1.0f ? 16 : 0);
        }
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) bits |= __shfl_xor(bits, off);
    if ((threadIdx.x & 63) == 0) wave_bits[threadIdx.x >> 6] = bits;
    __syncthreads();
    if (threadIdx.x == 0) {
        bits = wave_bits[0] | wave_bits[1] | wave_bits[2] | wave_bits[3];
        if (bits != 0) atomicOr(&flags[b], bits);
    }
}

// matplotlib's Normalize(0, vmax) and Colormap.__call__(bytes=True) on one value, float32 in its order; no branch.
// The clamp is the three range rules at once: xa == 256 -> 255 and xa >= 256 -> table[255] (the same entry), xa < 0 ->
// table[0]; v_max_f32 / v_min_f32 drop a NaN, so a NaN arrives at table[0] and is repainted where the image has no bad pixel.
__device__ __forceinline__ unsigned ri_viridis(const unsigned *table, float x, bool on, float vmax, bool any_bad) {
    const float v = on ? x : -1.0f;
    const float xa = (v / vmax) * 256.0f;
    unsigned c = table[(int)fminf(fmaxf(xa, 0.0f), 255.0f)];  // (int): truncation
    c = (xa != xa && !any_bad) ? RI_RED : c;
    return v == -1.0f ? RI_RED : c;  // masked_where(x == -1): an unmasked -1 too, a NaN not
}

// K19's classification as bytes; est and gt are already scaled
__device__ __forceinline__ unsigned ri_error(int kind, int y, int x, bool on, float est, float g, float abs_thres,
                                             float rel_thres) {
    int cls = on ? eimg_row(kind, eimg_scale(kind, fabsf(g - est), g, abs_thres, rel_thres)) : -1;
    cls = eimg_in_legend(y, x) ? x / 20 : cls;  // the legend last, over masked pixels too
    return cls >= 0 ? eimg_rgba[cls] : RI_BLACK;
}

// PX pixels of a row per thread.  PX = 4: W % 4 == 0 and every map 16-byte aligned row by row (the mask 4-byte), checked by
// the entry point -- 16-byte loads, a panel's four pixels in one 16-byte store.  PX = 1: any width, pitch and alignment,
// 4-byte loads and stores that a wave still coalesces.
template <int PX>
__global__ void __launch_bounds__(RI_BLOCK)
result_img_kernel(unsigned *__restrict__ out, const int *__restrict__ flags, const float *__restrict__ pred,
                  long long pred_row_stride, long long pred_img_stride, const float *__restrict__ gt_disp,
                  const float *__restrict__ gt_depth, const uint8_t *__restrict__ mask, const float *__restrict__ fb,
                  float max_disp, float depth_hi, float disp_abs_thres, float disp_rel_thres, float depth_scale,
                  float depth_abs_thres, int H, int W, int groups_per_row, long long total_groups) {
    static_assert(PX == 1 || PX == 4, "one pixel or one 16-byte store per panel");
    __shared__ unsigned table[256];
    {
        const unsigned char *c = az_viridis_rgb[threadIdx.x];  // RI_BLOCK == 256 rows
        table[threadIdx.x] = 0xff000000u | ((unsigned)c[2] << 16) | ((unsigned)c[1] << 8) | (unsigned)c[0];
    }
    __syncthreads();
    const size_t hw = (size_t)H * (size_t)W;
    for (long long t = (long long)blockIdx.x * RI_BLOCK + threadIdx.x; t < total_groups; t += (long long)gridDim.x * RI_BLOCK) {
        const long long row = t / groups_per_row;
        const int x0 = PX * (int)(t - row * groups_per_row);
        const int b = (int)(row / H), y = (int)(row - (long long)b * H);
        const size_t i0 = (size_t)row * (size_t)W + (size_t)x0;  // first pixel of the group in a contiguous [B,1,H,W] map
        const float *pp = ri_pred_row(pred, pred_row_stride, pred_img_stride, b, y) + x0;
        float pd[PX], gd[PX], gz[PX];
        unsigned mk;  // the group's mask bytes, pixel k in byte k
        if constexpr (PX == 4) {
            const float4 p4 = *reinterpret_cast<const float4 *>(pp), d4 = *reinterpret_cast<const float4 *>(gt_disp + i0),
                         z4 = *reinterpret_cast<const float4 *>(gt_depth + i0);
            pd[0] = p4.x; pd[1] = p4.y; pd[2] = p4.z; pd[3] = p4.w;
            gd[0] = d4.x; gd[1] = d4.y; gd[2] = d4.z; gd[3] = d4.w;
            gz[0] = z4.x; gz[1] = z4.y; gz[2] = z4.z; gz[3] = z4.w;
            mk = *reinterpret_cast<const unsigned *>(mask + i0);
        } else {
            pd[0] = pp[0]; gd[0] = gt_disp[i0]; gz[0] = gt_depth[i0];
            mk = mask[i0];
        }
        const float fbv = fb[b];
        const int fl = flags[b];
        unsigned c[6][PX];
#pragma unroll
        for (int k = 0; k < PX; ++k) {
            const bool on = ((mk >> (8 * k)) & 0xffu) != 0;
            const float pz = fbv / pd[k];  // test.py:209, the product made by the caller
            c[0][k] = ri_viridis(table, pd[k], on, max_disp, (fl & 1) != 0);
            c[1][k] = ri_viridis(table, gd[k], on, max_disp, (fl & 2) != 0);
            c[2][k] = ri_error(0, y, x0 + k, on, pd[k], gd[k], disp_abs_thres, disp_rel_thres);
            c[3][k] = ri_viridis(table, pz, on, depth_hi, (fl & 8) != 0);
            c[4][k] = ri_viridis(table, gz[k], on, depth_hi, (fl & 16) != 0);
            c[5][k] = ri_error(1, y, x0 + k, on, pz * depth_scale, gz[k] * depth_scale, depth_abs_thres, 0.0f);
        }
        unsigned *o = out + ((size_t)b * 6 * hw + (size_t)y * (size_t)W + (size_t)x0);
#pragma unroll
        for (int m = 0; m < 6; ++m) {
            if constexpr (PX == 4)
                *reinterpret_cast<uint4 *>(o + (size_t)m * hw) = make_uint4(c[m][0], c[m][1], c[m][2], c[m][3]);
            else
                o[(size_t)m * hw] = c[m][0];
        }
    }
}

static bool ri_multiple(const void *p, unsigned n) { return (reinterpret_cast<uintptr_t>(p) & (n - 1)) == 0; }

extern "C" int az_result_images(uint8_t *out, int32_t *flags, const float *pred_disp, long long pred_row_stride,
                                long long pred_img_stride, const float *gt_disp, const float *gt_depth, const uint8_t *mask,
                                const float *focal_x_baseline, float max_disp, float depth_hi, float disp_abs_thres,
                                float disp_rel_thres, float depth_scale, float depth_abs_thres, int B, int H, int W,
                                void *stream) {
    AZ_REQUIRE_PTR(out); AZ_REQUIRE_PTR(flags); AZ_REQUIRE_PTR(pred_disp); AZ_REQUIRE_PTR(gt_disp);
    AZ_REQUIRE_PTR(gt_depth); AZ_REQUIRE_PTR(mask); AZ_REQUIRE_PTR(focal_x_baseline);
    AZ_REQUIRE(B > 0 && H > 0 && W > 0);
    AZ_REQUIRE(pred_row_stride >= W && pred_img_stride >= 0);
    AZ_REQUIRE(max_disp > 0.0f && depth_hi > 0.0f);  // (a NaN fails both)
    AZ_REQUIRE(ri_multiple(out, 4));  // a pixel is stored as one 4-byte word
    hipStream_t s = az_stream(stream);
    if (hipMemsetAsync(flags, 0, (size_t)B * sizeof(int32_t), s) != hipSuccess) return AZ_ELAUNCH;
    const long long hw = (long long)H * W;
    long long bpi = (hw + RI_BLOCK - 1) / RI_BLOCK;
    const long long cap = B >= RI_FLAGS_GRID_CAP ? 1 : RI_FLAGS_GRID_CAP / B;
    if (bpi > cap) bpi = cap;
    if (bpi * B > 0x7fffffffLL) return AZ_EUNSUPPORTED;
    hipLaunchKernelGGL(result_flags_kernel, dim3((unsigned)(bpi * B)), dim3(RI_BLOCK), 0, s, flags, pred_disp,
                       pred_row_stride, pred_img_stride, gt_disp, gt_depth, mask, focal_x_baseline, H, W, (int)bpi);
    if (az_launch_status() != AZ_OK) return AZ_ELAUNCH;
    // four pixels per thread where every 16-byte access is aligned in every row of every image
    const bool wide = W % 4 == 0 && ri_multiple(out, 16) && ri_multiple(gt_disp, 16) && ri_multiple(gt_depth, 16) &&
                      ri_multiple(mask, 4) && ri_multiple(pred_disp, 16) && pred_row_stride % 4 == 0 &&
                      pred_img_stride % 4 == 0;
    const int gpr = wide ? W / 4 : W;
    const long long total = (long long)B * H * gpr;
    hipLaunchKernelGGL(wide ? result_img_kernel<4> : result_img_kernel<1>, dim3(az_grid_for(total, RI_BLOCK)), dim3(RI_BLOCK),
                       0, s, reinterpret_cast<unsigned *>(out), flags, pred_disp, pred_row_stride, pred_img_stride, gt_disp,
                       gt_depth, mask, focal_x_baseline, max_disp, depth_hi, disp_abs_thres, disp_rel_thres, depth_scale,
                       depth_abs_thres, H, W, gpr, total);
    return az_launch_status();
}
