// K19 -- colour-coded error images: reference utils/util.py:185-244 (depth_error_img, disp_error_img) with their colour
// tables (:143-182), which train.py:353-356 and test.py:244,260 run on the host after copying prediction, ground truth and
// mask there (eleven boolean-indexed numpy passes per image, on every training step).
// One thread per pixel, float32 throughout with IEEE division (no fast-math, no reciprocal): e = |gt - est| scaled by the
// thresholds, the table row with lower <= e < upper, its colour / 255; black where the mask is off or no row matches (NaN,
// +inf against the open last bin, a negative quotient); the legend over the top-left corner last.
// 9 bytes read and 12 written per pixel.
#include "az_common.h"

#define EIMG_ROWS 11
// the bounds as the reference's float32 tables hold them: Python doubles rounded once to float32
__constant__ float eimg_bounds[2][EIMG_ROWS + 1] = {
    {0.0f, (float)0.00001, (float)(0.1875 / 3.0), (float)(0.375 / 3.0), (float)(0.75 / 3.0), (float)(1.5 / 3.0),
     (float)(3 / 3.0), (float)(6 / 3.0), (float)(12 / 3.0), (float)(24 / 3.0), (float)(48 / 3.0), __builtin_inff()},
    {0.0f, (float)0.00001, (float)(2000.0 / 1024), (float)(2000.0 / 512), (float)(2000.0 / 256), (float)(2000.0 / 128),
     (float)(2000.0 / 64), (float)(2000.0 / 32), (float)(2000.0 / 16), (float)(2000.0 / 8), (float)(2000.0 / 4),
     __builtin_inff()}};
// both kinds share the colours; `cols[:, 2:5] /= 255.0` on a float32 array is a float32 division
#define EIMG_C(r, g, b) {r / 255.0f, g / 255.0f, b / 255.0f}
__constant__ float eimg_colour[EIMG_ROWS][3] = {
    EIMG_C(0.0f, 0.0f, 0.0f),       EIMG_C(49.0f, 54.0f, 149.0f),   EIMG_C(69.0f, 117.0f, 180.0f), EIMG_C(116.0f, 173.0f, 209.0f),
    EIMG_C(171.0f, 217.0f, 233.0f), EIMG_C(224.0f, 243.0f, 248.0f), EIMG_C(254.0f, 224.0f, 144.0f), EIMG_C(253.0f, 174.0f, 97.0f),
    EIMG_C(244.0f, 109.0f, 67.0f),  EIMG_C(215.0f, 48.0f, 39.0f),   EIMG_C(165.0f, 0.0f, 38.0f)};

__global__ void __launch_bounds__(256)
error_img_kernel(float *__restrict__ out, const float *__restrict__ est, const float *__restrict__ gt,
                 const uint8_t *__restrict__ mask, int kind, float abs_thres, float rel_thres, int layout, int H, int W,
                 long long total) {
    const long long hw = (long long)H * W;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long long)gridDim.x * 256) {
        const long long b = i / hw, p = i - b * hw;
        const int y = (int)(p / W), x = (int)(p - (long long)y * W);
        int cls = -1;
        if (y < 10 && x < 20 * EIMG_ROWS) {
            cls = x / 20;  // the legend, drawn over masked pixels too
        } else if (mask[i] != 0) {
            const float g = gt[i];
            float e = fabsf(g - est[i]);
            if (kind == 0) {
                const float a = e / abs_thres, r = (e / g) / rel_thres;
                e = a < r ? a : r;  // np.minimum: a NaN on either side wins (fminf would drop it)
                if (a != a) e = a;
                if (r != r) e = r;
            } else {
                e = e / abs_thres;
            }
            const float *bd = eimg_bounds[kind];
#pragma unroll
            for (int k = 0; k < EIMG_ROWS; ++k)
                if (e >= bd[k] && e < bd[k + 1]) cls = k;
        }
        float r = 0.0f, g = 0.0f, bl = 0.0f;
        if (cls >= 0) { r = eimg_colour[cls][0]; g = eimg_colour[cls][1]; bl = eimg_colour[cls][2]; }
        if (layout == 0) {
            float *o = out + 3 * i;
            o[0] = r; o[1] = g; o[2] = bl;
        } else {
            float *o = out + 3 * b * hw + p;
            o[0] = r; o[hw] = g; o[2 * hw] = bl;
        }
    }
}

extern "C" int az_error_img(float *out, const float *est, const float *gt, const uint8_t *mask, int kind, float abs_thres,
                            float rel_thres, int layout, int B, int H, int W, void *stream) {
    if (out == nullptr || est == nullptr || gt == nullptr || mask == nullptr) return AZ_EINVAL;
    AZ_REQUIRE(B > 0 && H > 0 && W > 0);
    AZ_REQUIRE((kind == 0 || kind == 1) && (layout == 0 || layout == 1));
    const long long total = (long long)B * H * W;
    hipLaunchKernelGGL(error_img_kernel, dim3(az_grid_for(total, 256)), dim3(256), 0, az_stream(stream), out, est, gt, mask,
                       kind, abs_thres, rel_thres, layout, H, W, total);
    return az_launch_status();
}
