// K21 -- the real domain's resize on the GPU: reference datasets/messytable.py:324-341 (the real images),
// :353-356 (the robot mask), :410-420 (the stored temporal pattern) call Pillow's Image.resize(size, resample=BILINEAR) on
// 8-bit grey images, per item, in a DataLoader worker.  Pillow's 8-bit path (ImagingResample) is fixed-point and two-pass:
//     horizontal  tmp[y][xx] = clip8((2^21 + sum_k img[y][first_x[xx] + k] coef_x[xx][k]) >> 22)   -- a uint8 image
//     vertical    out[yy][xx] = clip8((2^21 + sum_k tmp[first_y[yy] + k][xx] coef_y[yy][k]) >> 22)
// with the per-axis tables of az_resample_table.h (built on the host, handed over as device memory).  Integer arithmetic in a
// fixed order: the result is Pillow's, bit for bit, and the same from run to run.  The largest sum is 255 2^22 + 2^21 < 2^31.
// One launch does both passes for a batch and writes only the window [y0, y0 + h) x [x0, x0 + w) of the resized image (the
// loader's crop, messytable.py:366-398), as uint8 levels, as float32 v / 255 (a real division: the bits of the float32 image
// np.array(img) / 255), or as both.
// A 256-thread workgroup owns a 32 x 64 tile of the window.  It runs the horizontal pass for the source rows its vertical
// taps span (fewer than 32 * 8 + 17 at the ratio cap) into a uint8 LDS slab -- the rounded intermediate image IS the slab --
// then the vertical pass from the slab, four neighbouring pixels per thread, and stores them as one dword / float4 where
// the rows of the output start on such a boundary.  The horizontal work on the rows two vertically adjacent tiles share is
// done twice (at 720 -> 540: 45 slab rows for 32 output rows).  Source pixels are read as single bytes: the row starts are
// unaligned whenever Win % 4 != 0, and first_x moves by in / out per column.
// The tables are device memory the host cannot inspect: every source row and column index, count and slab index is clamped,
// so a corrupt table gives wrong pixels, never a read outside the image or the slab.
#include "az_common.h"
#include "az_resample_table.h"

#define RS_TW 64  // tile: 64 columns x 32 rows of the window, 256 threads
#define RS_TH 32
#define RS_TS (2 + AZ_RESAMPLE_MAX_KSIZE)  // ints per staged table row: 19, odd -- lanes reading a column hit distinct banks
#define RS_SLAB_ROWS (RS_TH * AZ_RESAMPLE_MAX_RATIO + AZ_RESAMPLE_MAX_KSIZE)

__device__ __forceinline__ int rs_clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }
__device__ __forceinline__ unsigned rs_round8(unsigned acc) {
    return (unsigned)rs_clampi((int)acc >> AZ_RESAMPLE_BITS, 0, 255);
}

// grid (tiles_x * tiles_y, N)
__global__ void __launch_bounds__(256)
resample_kernel(uint8_t *__restrict__ out_u8, float *__restrict__ out_f32, const uint8_t *__restrict__ img,
                const int32_t *__restrict__ table_y, const int32_t *__restrict__ table_x, int Hin, int Win, int ks_y,
                int ks_x, int y0, int x0, int h, int w, int tiles_x, int vec_u8, int vec_f32) {
    __shared__ int tab_x[RS_TW * RS_TS];
    __shared__ int tab_y[RS_TH * RS_TS];
    __shared__ __attribute__((aligned(16))) uint8_t slab[RS_SLAB_ROWS * RS_TW];
    const int tid = threadIdx.x;
    const int ty = blockIdx.x / tiles_x, tx = blockIdx.x - ty * tiles_x;
    const int wx0 = tx * RS_TW, wy0 = ty * RS_TH;  // the tile's corner inside the window
    const int rows = min(RS_TH, h - wy0);
    const uint8_t *p = img + (size_t)blockIdx.y * Hin * Win;

    // the table rows of the tile's columns and rows; a ragged tile repeats the window's last column / row
    for (int i = tid; i < RS_TW * (2 + ks_x); i += 256) {
        const int c = i / (2 + ks_x), e = i - c * (2 + ks_x);
        tab_x[c * RS_TS + e] = table_x[(size_t)(x0 + min(wx0 + c, w - 1)) * (2 + ks_x) + e];
    }
    for (int i = tid; i < RS_TH * (2 + ks_y); i += 256) {
        const int r = i / (2 + ks_y), e = i - r * (2 + ks_y);
        tab_y[r * RS_TS + e] = table_y[(size_t)(y0 + min(wy0 + r, h - 1)) * (2 + ks_y) + e];
    }
    __syncthreads();

    // slab row r holds source row min(src0 + r, Hin - 1), r < nrows
    const int src0 = rs_clampi(tab_y[0], 0, Hin - 1);
    const int *last_y = tab_y + (rows - 1) * RS_TS;
    const int src1 = rs_clampi(last_y[0], 0, Hin - 1) + rs_clampi(last_y[1], 0, ks_y);
    const int nrows = rs_clampi(src1 - src0, 1, RS_SLAB_ROWS);

    {  // horizontal pass: a wave per slab row, a lane per column (the same column in every round: 256 % 64 == 0)
        const int c = tid & (RS_TW - 1);
        const int *t = tab_x + c * RS_TS;
        const int first = rs_clampi(t[0], 0, Win - 1), count = rs_clampi(t[1], 0, ks_x);
        for (int r = tid >> 6; r < nrows; r += 4) {
            const uint8_t *row = p + (size_t)min(src0 + r, Hin - 1) * Win;
            unsigned acc = 1u << (AZ_RESAMPLE_BITS - 1);
            for (int k = 0; k < count; ++k) acc += (unsigned)row[min(first + k, Win - 1)] * (unsigned)t[2 + k];
            slab[r * RS_TW + c] = (uint8_t)rs_round8(acc);
        }
    }
    __syncthreads();

    // vertical pass: thread = 4 neighbouring columns of rows ry and ry + 16
    const int xq = tid & 15, ry = tid >> 4, wx = wx0 + 4 * xq;
#pragma unroll
    for (int it = 0; it < 2; ++it) {
        const int oy = ry + 16 * it;
        if (oy >= rows || wx >= w) continue;
        const int *t = tab_y + oy * RS_TS;
        const int r0 = rs_clampi(t[0], 0, Hin - 1) - src0, count = rs_clampi(t[1], 0, ks_y);
        unsigned acc[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[j] = 1u << (AZ_RESAMPLE_BITS - 1);
        for (int k = 0; k < count; ++k) {
            const int r = rs_clampi(r0 + k, 0, nrows - 1);
            const unsigned px = *reinterpret_cast<const unsigned *>(slab + r * RS_TW + 4 * xq);
            const unsigned cf = (unsigned)t[2 + k];
            acc[0] += (px & 255u) * cf;
            acc[1] += ((px >> 8) & 255u) * cf;
            acc[2] += ((px >> 16) & 255u) * cf;
            acc[3] += (px >> 24) * cf;
        }
        unsigned v[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) v[j] = rs_round8(acc[j]);
        const size_t o = ((size_t)blockIdx.y * h + (wy0 + oy)) * w + wx;
        if (out_u8 != nullptr) {
            if (vec_u8) {  // w % 4 == 0: wx + 3 < w
                *reinterpret_cast<unsigned *>(out_u8 + o) = v[0] | (v[1] << 8) | (v[2] << 16) | (v[3] << 24);
            } else {
#pragma unroll
                for (int j = 0; j < 4; ++j)
                    if (wx + j < w) out_u8[o + j] = (uint8_t)v[j];
            }
        }
        if (out_f32 != nullptr) {
            float q[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) q[j] = (float)v[j] / 255.f;  // a real division: the bits of float32(v / 255)
            if (vec_f32) {
                *reinterpret_cast<float4 *>(out_f32 + o) = make_float4(q[0], q[1], q[2], q[3]);
            } else {
#pragma unroll
                for (int j = 0; j < 4; ++j)
                    if (wx + j < w) out_f32[o + j] = q[j];
            }
        }
    }
}

extern "C" int az_resample_bilinear_ksize(int in_size, int out_size) { return az_resample_ksize(in_size, out_size); }

extern "C" int az_resample_bilinear_table(int32_t *table, int in_size, int out_size) {
    return az_resample_table(table, in_size, out_size);
}

extern "C" int az_resize_bilinear_u8(uint8_t *out_u8, float *out_f32, const uint8_t *img, const int32_t *table_y,
                                     const int32_t *table_x, int N, int Hin, int Win, int Hout, int Wout, int y0, int x0,
                                     int h, int w, void *stream) {
    if (img == nullptr || table_y == nullptr || table_x == nullptr) return AZ_EINVAL;
    if (out_u8 == nullptr && out_f32 == nullptr) return AZ_EINVAL;
    if (N <= 0 || h <= 0 || w <= 0 || y0 < 0 || x0 < 0) return AZ_EINVAL;
    const int ks_y = az_resample_ksize(Hin, Hout), ks_x = az_resample_ksize(Win, Wout);
    if (ks_y == AZ_EINVAL || ks_x == AZ_EINVAL) return AZ_EINVAL;  // a non-positive size
    if (ks_y < 0 || ks_x < 0) return AZ_EUNSUPPORTED;              // a ratio above 8 (on an axis of more than 17 pixels)
    if ((long long)y0 + h > Hout || (long long)x0 + w > Wout) return AZ_EINVAL;
    if ((long long)Hin * Win > 0x7fffffffLL || N > 65535) return AZ_EUNSUPPORTED;
    const int tiles_x = (w + RS_TW - 1) / RS_TW;
    const long long tiles = (long long)tiles_x * ((h + RS_TH - 1) / RS_TH);
    if (tiles > 0x7fffffffLL) return AZ_EUNSUPPORTED;
    // four pixels per store where every row of every output image starts on a vector boundary
    const int vec_u8 = w % 4 == 0 && (uintptr_t)out_u8 % 4 == 0;
    const int vec_f32 = w % 4 == 0 && (uintptr_t)out_f32 % 16 == 0;
    hipLaunchKernelGGL(resample_kernel, dim3((unsigned)tiles, N), dim3(256), 0, az_stream(stream), out_u8, out_f32, img,
                       table_y, table_x, Hin, Win, ks_y, ks_x, y0, x0, h, w, tiles_x, vec_u8, vec_f32);
    return az_launch_status();
}
