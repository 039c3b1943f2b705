// K19 -- colour-coded error images: reference utils/util.py:185-244 (depth_error_img, disp_error_img) with their colour
// tables (:143-182), which train.py:353-356 and test.py:244,260 run on the host after copying prediction, ground truth and
// mask there (eleven boolean-indexed numpy passes per image, on every training step).
// One thread per pixel, float32 throughout with IEEE division (no fast-math, no reciprocal): e = |gt - est| scaled by the
// thresholds, the table row with lower <= e < upper, its colour / 255; black where the mask is off or no row matches (NaN,
// +inf against the open last bin, a negative quotient); the legend over the top-left corner last.
// 9 bytes read and 12 written per pixel.
#include "az_error_table.h"

__global__ void __launch_bounds__(256)
error_img_kernel(float *__restrict__ out, const float *__restrict__ est, const float *__restrict__ gt,
                 const uint8_t *__restrict__ mask, int kind, float abs_thres, float rel_thres, int layout, int H, int W,
                 long long total) {
    const long long hw = (long long)H * W;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long long)gridDim.x * 256) {
        const long long b = i / hw, p = i - b * hw;
        const int y = (int)(p / W), x = (int)(p - (long long)y * W);
        int cls = -1;
        if (eimg_in_legend(y, x)) {
            cls = x / 20;  // the legend, drawn over masked pixels too
        } else if (mask[i] != 0) {
            const float g = gt[i];
            cls = eimg_row(kind, eimg_scale(kind, fabsf(g - est[i]), g, abs_thres, rel_thres));
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
