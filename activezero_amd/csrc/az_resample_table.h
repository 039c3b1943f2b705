// The per-axis coefficient tables of K21 (az_resample.hip): what Pillow's ImagingResample builds for the triangle
// ("BILINEAR", support 1.0) filter and 8-bit data -- precompute_coeffs followed by normalize_coeffs_8bpc -- step by step in
// double, in Pillow's order of operations.  Free of HIP types, like az_launch_math.h, so that the SAME functions the library
// exports are also compiled with g++ -fsanitize=address,undefined and swept over sizes on the CPU
// (tests/host/resample_table_test.cpp, tests/test_resample_table_cpu.py).
//
//   scale = in / out;  fs = max(scale, 1);  support = 1.0 * fs;  ss = 1 / fs;  ksize = (int)ceil(support) * 2 + 1
//   per output index xx:  center = (xx + 0.5) * scale
//                         first  = max((int)(center - support + 0.5), 0),  last = min((int)(center + support + 0.5), in)
//                         w[x]   = tri((x + first - center + 0.5) * ss), x < count = last - first;  tri(a) = max(1 - |a|, 0)
//                         w[x]  /= w[0] + w[1] + ... (in that order) unless the sum is zero
//                         coef[x] = (int)(0.5 + w[x] * 2^22), zero from count to ksize
// A table is [out][2 + ksize] int32: first, count, coef[0 .. ksize).  in == out gives the identity (one tap of 2^22).
// Supported: in <= 8 out (ksize <= 17), and any in <= 17 whatever the ratio -- count never exceeds in, so the rows of such an
// axis fit 17 taps too, and their table is laid out with ksize = 17.
#pragma once
#include <math.h>
#include <stdint.h>

#include "../../include/azhip.h"

// A fused (xx + 0.5) * scale or x / ww would round once where Pillow rounds twice and can move a coefficient by one unit.
#if defined(__clang__)
#pragma clang fp contract(off)
#elif defined(__GNUC__)
#pragma GCC push_options
#pragma GCC optimize("fp-contract=off")
#endif

#define AZ_RESAMPLE_BITS 22       // Pillow's PRECISION_BITS for 8-bit data: 32 - 8 - 2
#define AZ_RESAMPLE_MAX_RATIO 8   // in <= 8 out
#define AZ_RESAMPLE_MAX_KSIZE 17  // (int)ceil(8.0) * 2 + 1

// taps per table row; AZ_EINVAL for a non-positive size, AZ_EUNSUPPORTED for in > 8 out unless in <= 17
inline int az_resample_ksize(int in_size, int out_size) {
    if (in_size <= 0 || out_size <= 0) return AZ_EINVAL;
    if ((long long)in_size > (long long)AZ_RESAMPLE_MAX_RATIO * out_size)
        return in_size <= AZ_RESAMPLE_MAX_KSIZE ? AZ_RESAMPLE_MAX_KSIZE : AZ_EUNSUPPORTED;
    const double scale = (double)in_size / (double)out_size;
    const double support = 1.0 * (scale < 1.0 ? 1.0 : scale);
    return (int)ceil(support) * 2 + 1;
}

// table: out_size * (2 + ksize) int32, all written.  Returns 0 or the code of az_resample_ksize.
inline int az_resample_table(int32_t *table, int in_size, int out_size) {
    const int ksize = az_resample_ksize(in_size, out_size);
    if (ksize < 0) return ksize;
    if (table == nullptr) return AZ_EINVAL;
    const double scale = (double)in_size / (double)out_size;
    const double filterscale = scale < 1.0 ? 1.0 : scale;
    const double support = 1.0 * filterscale;
    const double ss = 1.0 / filterscale;
    double w[AZ_RESAMPLE_MAX_KSIZE];
    for (int xx = 0; xx < out_size; ++xx) {
        int32_t *row = table + (long long)xx * (2 + ksize);
        const double center = (xx + 0.5) * scale;
        int first = (int)(center - support + 0.5);
        if (first < 0) first = 0;
        int last = (int)(center + support + 0.5);
        if (last > in_size) last = in_size;
        const int count = last - first;  // <= min(2 support + 1, in) <= ksize
        double ww = 0.0;
        for (int x = 0; x < count; ++x) {
            double a = (x + first - center + 0.5) * ss;
            if (a < 0.0) a = -a;
            w[x] = a < 1.0 ? 1.0 - a : 0.0;
            ww += w[x];
        }
        row[0] = first;
        row[1] = count;
        for (int x = 0; x < ksize; ++x) {
            if (x < count) {
                const double v = ww != 0.0 ? w[x] / ww : w[x];
                row[2 + x] = (int32_t)(0.5 + v * (double)(1 << AZ_RESAMPLE_BITS));  // the weights are never negative
            } else {
                row[2 + x] = 0;
            }
        }
    }
    return AZ_OK;
}

#if !defined(__clang__) && defined(__GNUC__)
#pragma GCC pop_options
#endif
