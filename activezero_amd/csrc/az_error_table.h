// The error colour tables of the reference's utils/util.py:143-182 (gen_error_colormap_disp / _depth) and the search for a
// scaled error's row (:185-244), stated ONCE for K19 az_error_img (az_error_img.hip: float colours) and K24
// az_result_images (az_result_img.hip: the same rows as bytes).  tests/_gt_prep_ref.py restates them in numpy.
#pragma once
#include "az_common.h"

#define EIMG_ROWS 11
// the bounds as the reference's float32 tables hold them: Python doubles rounded once to float32
static __constant__ float eimg_bounds[2][EIMG_ROWS + 1] = {
    {0.0f, (float)0.00001, (float)(0.1875 / 3.0), (float)(0.375 / 3.0), (float)(0.75 / 3.0), (float)(1.5 / 3.0),
     (float)(3 / 3.0), (float)(6 / 3.0), (float)(12 / 3.0), (float)(24 / 3.0), (float)(48 / 3.0), __builtin_inff()},
    {0.0f, (float)0.00001, (float)(2000.0 / 1024), (float)(2000.0 / 512), (float)(2000.0 / 256), (float)(2000.0 / 128),
     (float)(2000.0 / 64), (float)(2000.0 / 32), (float)(2000.0 / 16), (float)(2000.0 / 8), (float)(2000.0 / 4),
     __builtin_inff()}};
// both kinds share the colours, 0..255 per component
#define EIMG_RGB(X)                                                                                                      \
    X(0, 0, 0) X(49, 54, 149) X(69, 117, 180) X(116, 173, 209) X(171, 217, 233) X(224, 243, 248) X(254, 224, 144)         \
    X(253, 174, 97) X(244, 109, 67) X(215, 48, 39) X(165, 0, 38)
// K19: `cols[:, 2:5] /= 255.0` on a float32 array is a float32 division
#define EIMG_C(r, g, b) {(float)(r) / 255.0f, (float)(g) / 255.0f, (float)(b) / 255.0f},
static __constant__ float eimg_colour[EIMG_ROWS][3] = {EIMG_RGB(EIMG_C)};
// K24: the integers themselves as R, G, B, A = 255 bytes in memory order.  plt.imsave's (c * 255).astype(uint8) on K19's
// float32 k / 255 gives k back for every k of the table (tests/test_result_images_cpu.py)
#define EIMG_P(r, g, b) (0xff000000u | ((unsigned)(b) << 16) | ((unsigned)(g) << 8) | (unsigned)(r)),
static __constant__ unsigned eimg_rgba[EIMG_ROWS] = {EIMG_RGB(EIMG_P)};

// the legend: rows < 10, columns [20 i, 20 i + 20) take row i, over masked pixels too
__device__ __forceinline__ bool eimg_in_legend(int y, int x) { return y < 10 && x < 20 * EIMG_ROWS; }

// e = |gt - est| scaled by the thresholds; kind 0 = disparity, 1 = depth
__device__ __forceinline__ float eimg_scale(int kind, float e, float g, float abs_thres, float rel_thres) {
    if (kind == 0) {
        const float a = e / abs_thres, r = (e / g) / rel_thres;
        e = a < r ? a : r;  // np.minimum: a NaN on either side wins (fminf would drop it)
        if (a != a) e = a;
        if (r != r) e = r;
        return e;
    }
    return e / abs_thres;
}

// the table row with lower <= e < upper, -1 where none matches (NaN, +inf against the open last bin, a negative quotient)
__device__ __forceinline__ int eimg_row(int kind, float e) {
    const float *bd = eimg_bounds[kind];
    int cls = -1;
#pragma unroll
    for (int k = 0; k < EIMG_ROWS; ++k)
        if (e >= bd[k] && e < bd[k + 1]) cls = k;
    return cls;
}
