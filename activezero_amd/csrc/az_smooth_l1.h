// The gradient clamp of the smooth-L1 losses, stated ONCE for K12 (az_disp_loss.hip) and K29 (az_ms_loss.hip).
#pragma once
#include "az_common.h"

// clamp(d, -1, 1) that keeps a NaN, as the autograd gradient of smooth-L1 does (fminf / fmaxf would give -1)
__device__ __forceinline__ float dl_clamp1(float d) { return az_min_nan(az_max_nan(d, -1.f), 1.f); }
