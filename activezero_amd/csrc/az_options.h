// The library's A/B switches (DESIGN.md section 4, table "A/B switches"): environment variables read ONCE, when the first
// call needs one, into one immutable struct -- no getenv in a launch path, no unsynchronised first-write caches
// (C++11 guarantees the initialisation of the function-local static in az_options() happens exactly once, under a lock).
#pragma once

// Every switch, once: X(field, environment variable, default, what it selects).  The struct below, its initialiser and the
// name table of az_option() (az_misc.hip) are generated from this list; DESIGN.md's table and tests/test_gpu_switches.py
// follow it (tests/test_options_cpu.py).
#define AZ_OPTION_LIST(X)                                                                                                            \
    X(conv2d_wgrad_r16, AZ_CONV2D_WGRAD_R16, 1, "1: 3x3 32/64-channel 2-D weight gradients on az_conv2d_wgrad16.hip")                 \
    X(conv_m128, AZ_CONV_M128, 1, "1: bf16x6 (precision 1) stride-1 32-output layers on az_conv3d_m128.hip")                         \
    X(conv_map, AZ_CONV_MAP, 2, "block -> tile map of the 3-D kernels: 0 linear, 1 XCD-chunked, 2 + banded (out of range: 2)")       \
    X(roll_seglen, AZ_ROLL_SEGLEN, 0, "> 0: depth-segment length of az_conv3d_roll.hip (0: chosen per launch)")                      \
    X(wgrad_slots, AZ_WGRAD_SLOTS, 256 * 8, "resident waves a 3-D one-kd-per-wave weight gradient may take")                         \
    X(wgrad_order, AZ_WGRAD_ORDER, 1, "work-list order of those kernels (1: XCD-chunked, depth fastest)")                            \
    X(wgrad_r16, AZ_WGRAD_R16, 2, "0 / 1 / 2: stride-1 3-D weight gradients on az_conv3d_wgrad16.hip (none / 32x32 / all)")          \
    X(wgrad_r16_wgs, AZ_WGRAD_R16_WGS, 0, "> 0: cap on that kernel's persistent workgroups")                                         \
    X(wgrad_r16_xcd, AZ_WGRAD_R16_XCD, 1, "1: that kernel's columns in XCD-contiguous runs")                                         \
    X(wgrad_s2r16, AZ_WGRAD_S2R16, 1, "1: f16x3 stride-2 3-D weight gradients on az_conv3d_wgrad16s2.hip")                           \
    X(conv_t2roll, AZ_CONV_T2ROLL, 1, "1: f16x3 transposed 64 -> 32 layers on az_conv3d_t2roll.hip")                                 \
    X(conv_s2roll, AZ_CONV_S2ROLL, 1, "1: f16x3 stride-2 32 -> 64 layers on az_conv3d_s2roll.hip (0: az_conv3d.hip's gather kernel)") \
    X(s2roll_seglen, AZ_S2ROLL_SEGLEN, 0, "> 0: output planes per depth segment of az_conv3d_s2roll.hip (0: chosen per launch)")     \
    X(conv_roll64, AZ_CONV_ROLL64, 1, "1: f16x3 stride-1 64 -> 64 layers on az_conv3d_roll.hip, two workgroups per patch")           \
    X(patch_tiled, AZ_PATCH_TILED, 1, "1: band-tiled patch-reprojection kernel (0: the per-pixel one)")

struct AzOptions {
#define AZ_OPTION_FIELD(field, env, dflt, doc) int field;
    AZ_OPTION_LIST(AZ_OPTION_FIELD)
#undef AZ_OPTION_FIELD
};

const AzOptions &az_options();
