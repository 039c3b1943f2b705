// K20 -- the loader's augmentation on the GPU: reference datasets/dataset_utils.py:49-83
// data_augmentation, applied by datasets/messytable.py:264-280, 402-404 to every image that enters the network.  The
// reference runs it per item, in float64, on three identical copies of a grey image, in a DataLoader worker:
//     GaussianBlur(ks, sigma)   k = exp(-0.5 (t / sigma)^2), t = -(ks-1)/2 .. (ks-1)/2, k /= sum k; the 2-D kernel is
//                               outer(k, k), the border mode "reflect" (the edge pixel is not repeated)
//     ColorJitter(b, c)         brightness clamp(b x, 0, 1) and contrast clamp(c x + (1 - c) m, 0, 1), m the mean over the
//                               image of 0.2989 r + 0.587 g + 0.114 b (0.9999 x for a grey image), in a random order
//     Normalize                 out[ch] = (x - mean[ch]) / std[ch], the ImageNet constants
// One kernel template, three modes: a statistics pass (one partial sum of the grey mean per workgroup, in the workspace
// slot of its tile), the apply pass after it, and the apply pass of a call without jitter.  Both passes RECOMPUTE the
// separable blur from the input through an LDS tile with a halo of ks / 2: 2 ks multiply-adds per pixel.
// Algorithmic bytes per pixel: jitter on 2 sizeof(in) + 12 (14 for uint8, 20 for float32); jitter off sizeof(in) + 12 (one
// launch; with both flags clear a streaming pass that touches no LDS).  Storing the blurred plane instead would cost
// sizeof(in) + 4 + 4 + 12.
// The mean is reproducible bit for bit and independent of B: no float atomics, a workgroup writes the fp32 sum of its
// tile into a fixed slot, the apply pass adds the image's slots in fp64 in a fixed order (thread t takes slots t, t + 256,
// ..., then the butterfly, then the four waves in order).
#include "az_common.h"

#define AUG_TW 64  // tile: 64 x 32 pixels, 256 threads, one thread = 4 neighbouring pixels of rows ry and ry + 16
#define AUG_TH 32
#define AUG_MAX_KS 31
#define AUG_HEAD 128  // floats in front of the tile: 32 doubles (the fp64 taps), 4 doubles and 4 floats (wave sums), 32 fp32 taps

template <int VEC> __device__ __forceinline__ void aug_load(const float *p, float (&v)[VEC]) {
    if constexpr (VEC == 4) {
        const float4 t = *reinterpret_cast<const float4 *>(p);
        v[0] = t.x; v[1] = t.y; v[2] = t.z; v[3] = t.w;
    } else {
        v[0] = p[0];
    }
}
// grey levels 0..255 become v / 255 with a real division: the bits of the float32 image u8 / 255
template <int VEC> __device__ __forceinline__ void aug_load(const uint8_t *p, float (&v)[VEC]) {
    if constexpr (VEC == 4) {
        const unsigned t = *reinterpret_cast<const unsigned *>(p);
        v[0] = (float)(t & 255u) / 255.f; v[1] = (float)((t >> 8) & 255u) / 255.f;
        v[2] = (float)((t >> 16) & 255u) / 255.f; v[3] = (float)(t >> 24) / 255.f;
    } else {
        v[0] = (float)p[0] / 255.f;
    }
}
template <typename IN_T> __device__ __forceinline__ float aug_load1(const IN_T *p) {
    float v[1];
    aug_load<1>(p, v);
    return v[0];
}

// "reflect" padding for an index at most n - 1 outside [0, n)
__device__ __forceinline__ int aug_reflect(int i, int n) { return i < 0 ? -i : (i >= n ? 2 * (n - 1) - i : i); }
// torch.clamp: NaN stays NaN
__device__ __forceinline__ float aug_clamp01(float v) { return v < 0.f ? 0.f : (v > 1.f ? 1.f : v); }

// MODE 0: statistics (partial[img * ntiles + tile] = sum of the grey values the contrast stage will average);
// MODE 1: apply with jitter (reads the image's partials); MODE 2: apply without jitter.
// grid (ntiles, B): one image per blockIdx.y, so the order branch is uniform in a workgroup.
template <typename IN_T, bool BLUR, int MODE>
__global__ void __launch_bounds__(256)
aug_kernel(float *__restrict__ out, float *__restrict__ partial, const IN_T *__restrict__ in,
           const float *__restrict__ params, int H, int W, int ks, int tiles_x, int vec_in, int vec_out) {
    extern __shared__ float4 aug_lds4[];
    float *lds = reinterpret_cast<float *>(aug_lds4);
    double *tap64 = reinterpret_cast<double *>(lds), *wave64 = tap64 + 32;
    float *wave32 = lds + 72, *tap = lds + 96;
    const int tid = threadIdx.x, img = blockIdx.y, ntiles = gridDim.x;
    const int ty = blockIdx.x / tiles_x, x0 = (blockIdx.x - ty * tiles_x) * AUG_TW, y0 = ty * AUG_TH;
    const IN_T *p = in + (size_t)img * H * W;
    const int r = ks >> 1, SW = AUG_TW + 2 * r, SH = AUG_TH + 2 * r;
    float *st = lds + AUG_HEAD, *rs = st + SH * SW;

    float sigma = 0.f, bright = 1.f, contrast = 1.f;
    bool contrast_first = false;
    if constexpr (BLUR) sigma = params[4 * img];
    if constexpr (MODE != 2) {
        bright = params[4 * img + 1];
        contrast = params[4 * img + 2];
        contrast_first = params[4 * img + 3] != 0.f;
    }

    if constexpr (BLUR) {
        // the taps in fp64 from the image's sigma, rounded to fp32 once; sigma <= 0: the limit, the identity
        if (tid < ks) {
            const double t = (double)(tid - r) / (double)sigma;
            tap64[tid] = sigma <= 0.f ? (tid == r ? 1.0 : 0.0) : exp(-0.5 * t * t);
        }
        __syncthreads();
        if (tid < ks) {
            double s = 0.0;
            for (int k = 0; k < ks; ++k) s += tap64[k];
            tap[tid] = (float)(tap64[tid] / s);
        }
        // the tile with its halo, [SH][SW].  Cells whose pixel lies more than r beyond the image (ragged tiles) feed no
        // output of the image: they are not loaded -- reflecting them could leave the image -- and hold zero.
        for (int i = tid; i < SH * 16; i += 256) {  // the 64 columns of the tile itself, four at a time
            const int ly = i >> 4, gyr = y0 - r + ly, gx = x0 + 4 * (i & 15);
            float v[4] = {0.f, 0.f, 0.f, 0.f};
            if (gyr < H + r) {
                const IN_T *row = p + (size_t)aug_reflect(gyr, H) * W;
                if (vec_in && gx < W) {  // W % 4 == 0: gx + 3 < W
                    aug_load<4>(row + gx, v);
                } else {
#pragma unroll
                    for (int j = 0; j < 4; ++j)
                        if (gx + j < W + r) v[j] = aug_load1(row + aug_reflect(gx + j, W));
                }
            }
            float *d = st + ly * SW + r + 4 * (i & 15);
            d[0] = v[0]; d[1] = v[1]; d[2] = v[2]; d[3] = v[3];
        }
        for (int i = tid; i < SH * 2 * r; i += 256) {  // the r columns on either side
            const int ly = i / (2 * r), c = i - ly * 2 * r, lx = c < r ? c : c + AUG_TW;
            const int gyr = y0 - r + ly, gxr = x0 - r + lx;
            float v = 0.f;
            if (gyr < H + r && gxr < W + r) v = aug_load1(p + (size_t)aug_reflect(gyr, H) * W + aug_reflect(gxr, W));
            st[ly * SW + lx] = v;
        }
        __syncthreads();
        for (int i = tid; i < SH * AUG_TW; i += 256) {  // horizontal pass: lanes along x, conflict-free
            const float *s = st + (i >> 6) * SW + (i & 63);
            float a = 0.f;
            for (int k = 0; k < ks; ++k) a = fmaf(tap[k], s[k], a);
            rs[i] = a;
        }
        __syncthreads();
    }

    const int xq = tid & 15, ry = tid >> 4, gx = x0 + 4 * xq;
    const float mean[3] = {0.485f, 0.456f, 0.406f}, stdv[3] = {0.229f, 0.224f, 0.225f};
    float grey_mean = 0.f, sum = 0.f;
    if constexpr (MODE == 1) {
        double s = 0.0;
        for (int i = tid; i < ntiles; i += 256) s += (double)partial[(size_t)img * ntiles + i];
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o);
        if ((tid & 63) == 0) wave64[tid >> 6] = s;
        __syncthreads();
        grey_mean = (float)((((wave64[0] + wave64[1]) + wave64[2]) + wave64[3]) / (double)(H * W));
    }
#pragma unroll
    for (int it = 0; it < 2; ++it) {
        const int oy = ry + 16 * it, gy = y0 + oy;
        float v[4] = {0.f, 0.f, 0.f, 0.f};
        if constexpr (BLUR) {  // vertical pass: one 16-byte LDS read per tap
            for (int k = 0; k < ks; ++k) {
                const float4 t = *reinterpret_cast<const float4 *>(rs + (oy + k) * AUG_TW + 4 * xq);
                const float w = tap[k];
                v[0] = fmaf(w, t.x, v[0]); v[1] = fmaf(w, t.y, v[1]); v[2] = fmaf(w, t.z, v[2]); v[3] = fmaf(w, t.w, v[3]);
            }
        } else if (gy < H) {
            const IN_T *row = p + (size_t)gy * W;
            if (vec_in && gx < W) {
                aug_load<4>(row + gx, v);
            } else {
#pragma unroll
                for (int j = 0; j < 4; ++j)
                    if (gx + j < W) v[j] = aug_load1(row + gx + j);
            }
        }
        if constexpr (MODE != 2) {
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                if (!contrast_first) v[j] = aug_clamp01(bright * v[j]);
                if constexpr (MODE == 0) {
                    // the three-term grey value of r = g = b: its weights sum to 0.9999
                    const float g = fmaf(0.114f, v[j], fmaf(0.587f, v[j], 0.2989f * v[j]));
                    if (gy < H && gx + j < W) sum += g;
                } else {
                    v[j] = aug_clamp01(fmaf(contrast, v[j], (1.f - contrast) * grey_mean));
                    if (contrast_first) v[j] = aug_clamp01(bright * v[j]);
                }
            }
        }
        if constexpr (MODE != 0) {
            if (gy < H) {
                float *o = out + ((size_t)img * 3 * H + gy) * W + gx;
#pragma unroll
                for (int ch = 0; ch < 3; ++ch, o += (size_t)H * W) {
                    float q[4];
#pragma unroll
                    for (int j = 0; j < 4; ++j) q[j] = (v[j] - mean[ch]) / stdv[ch];  // a real division: torch's bits
                    if (vec_out && gx < W) {
                        *reinterpret_cast<float4 *>(o) = make_float4(q[0], q[1], q[2], q[3]);
                    } else {
#pragma unroll
                        for (int j = 0; j < 4; ++j)
                            if (gx + j < W) o[j] = q[j];
                    }
                }
            }
        }
    }
    if constexpr (MODE == 0) {
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) sum += __shfl_xor(sum, o);
        if ((tid & 63) == 0) wave32[tid >> 6] = sum;
        __syncthreads();
        if (tid == 0) partial[(size_t)img * ntiles + blockIdx.x] = ((wave32[0] + wave32[1]) + wave32[2]) + wave32[3];
    }
}

static inline int aug_tiles_x(int W) { return (W + AUG_TW - 1) / AUG_TW; }
static inline long long aug_tiles(int H, int W) { return (long long)aug_tiles_x(W) * ((H + AUG_TH - 1) / AUG_TH); }

extern "C" long long az_augment_workspace(int B, int H, int W, int ks) {
    if (B <= 0 || H <= 0 || W <= 0) return AZ_EINVAL;
    if (ks < 3 || ks > AUG_MAX_KS || (ks & 1) == 0) return AZ_EUNSUPPORTED;
    if (H <= ks / 2 || W <= ks / 2) return AZ_EINVAL;  // a single reflection must suffice
    if ((long long)H * W > 0x7fffffffLL || B > 65535) return AZ_EUNSUPPORTED;
    return (B * aug_tiles(H, W) * 4 + 255) / 256 * 256;  // one fp32 partial sum per tile and image
}

template <typename IN_T, bool BLUR, int MODE>
static void aug_launch(float *out, float *partial, const void *img, const float *params, int B, int H, int W, int ks,
                       hipStream_t s) {
    const IN_T *in = static_cast<const IN_T *>(img);
    const int r = ks / 2;
    const size_t lds = (AUG_HEAD + (BLUR ? (size_t)(AUG_TH + 2 * r) * (2 * AUG_TW + 2 * r) : 0)) * sizeof(float);
    // four pixels per load / store where every row of every image starts on a vector boundary
    const int vec_in = W % 4 == 0 && (uintptr_t)img % (4 * sizeof(IN_T)) == 0;
    const int vec_out = W % 4 == 0 && (uintptr_t)out % 16 == 0;
    hipLaunchKernelGGL((aug_kernel<IN_T, BLUR, MODE>), dim3((unsigned)aug_tiles(H, W), B), dim3(256), lds, s, out, partial,
                       in, params, H, W, ks, aug_tiles_x(W), vec_in, vec_out);
}

template <typename IN_T>
static void aug_dispatch(float *out, float *partial, const void *img, const float *params, int B, int H, int W, int ks,
                         int flags, hipStream_t s) {
    const bool blur = flags & 1;
    if (flags & 2) {  // jitter: the statistics pass, then the apply pass
        if (blur) {
            aug_launch<IN_T, true, 0>(out, partial, img, params, B, H, W, ks, s);
            aug_launch<IN_T, true, 1>(out, partial, img, params, B, H, W, ks, s);
        } else {
            aug_launch<IN_T, false, 0>(out, partial, img, params, B, H, W, ks, s);
            aug_launch<IN_T, false, 1>(out, partial, img, params, B, H, W, ks, s);
        }
    } else if (blur) {
        aug_launch<IN_T, true, 2>(out, partial, img, params, B, H, W, ks, s);
    } else {
        aug_launch<IN_T, false, 2>(out, partial, img, params, B, H, W, ks, s);
    }
}

extern "C" int az_augment(float *out, float *workspace, long long workspace_bytes, const void *img, int img_is_u8,
                          const float *params, int B, int H, int W, int ks, int flags, void *stream) {
    if (out == nullptr || workspace == nullptr || img == nullptr) return AZ_EINVAL;
    if (flags < 0 || flags > 3 || (flags != 0 && params == nullptr)) return AZ_EINVAL;
    const long long need = az_augment_workspace(B, H, W, ks);
    if (need < 0) return (int)need;
    if (workspace_bytes < need) return AZ_EWORKSPACE;
    hipStream_t s = az_stream(stream);
    if (img_is_u8)
        aug_dispatch<uint8_t>(out, workspace, img, params, B, H, W, ks, flags, s);
    else
        aug_dispatch<float>(out, workspace, img, params, B, H, W, ks, flags, s);
    return az_launch_status();
}
