// The per-pixel terms of the disparity / depth error metrics (reference utils/cascade_metrics.py:16-62), stated ONCE for
// K12 az_disp_metrics (az_disp_loss.hip: sums over a whole batch) and K22 az_obj_metrics (az_obj_metrics.hip: the same
// sums per image and object label): the accumulator slots, the float32 expressions, the NaN-keeping clip and the
// thresholds.  tests/_reduce_ref.py restates them per pixel (k12_metrics).
#pragma once
#include "az_common.h"

// accumulator slots (dd = disparity error, dz = depth error in m)
enum {
    AZ_DM_EPE = 0,    // sum |dd|
    AZ_DM_BAD1 = 1,   // #(|dd| > 1)
    AZ_DM_BAD2 = 2,   // #(|dd| > 2)
    AZ_DM_MM = 3,     // sum clip(|1000 dz|, 0, 100)
    AZ_DM_Z2 = 4,     // #(|dz| > 2e-3)
    AZ_DM_Z4 = 5,     // #(|dz| > 4e-3)
    AZ_DM_Z8 = 6,     // #(|dz| > 8e-3)
    AZ_DM_COUNT = 7,  // masked pixels
    AZ_DM_SLOTS = 8
};

// the two float32 sums' terms and the five threshold tests of one pixel
struct az_dm_px {
    float dd, dmm;
    bool bad1, bad2, z2, z4, z8;
};

// cascade_metrics.py:36-37: depth_pred = focal_length * baseline / disp_pred (metres), IEEE float32 division
__device__ __forceinline__ float az_dm_depth(float fb, float disp_pred) { return fb / disp_pred; }

__device__ __forceinline__ az_dm_px az_dm_pixel(float disp_gt, float depth_gt, float disp_pred, float depth_pred) {
    az_dm_px p;
    p.dd = fabsf(disp_gt - disp_pred);
    const float dz = fabsf(depth_gt - depth_pred);
    // torch.clip: NaN stays, inf -> 100
    p.dmm = az_min_nan(az_max_nan(fabsf(depth_gt * 1000.f - depth_pred * 1000.f), 0.f), 100.f);
    p.bad1 = p.dd > 1.f;
    p.bad2 = p.dd > 2.f;
    p.z2 = dz > 2e-3f;
    p.z4 = dz > 4e-3f;
    p.z8 = dz > 8e-3f;
    return p;
}
