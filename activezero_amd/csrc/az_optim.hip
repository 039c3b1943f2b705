// K27 / K28: the optimizer step (include/azhip.h; activezero_amd/optim.py) -- Adam / AdamW over all tensors of a parameter
// group in one launch, with the global gradient norm, the clip coefficient, the scaler's inverse scale and the skip on
// non-finite gradients folded in.  Three launches: az_grad_sumsq_multi (only when a norm is wanted), az_optim_begin (one
// workgroup: the norm, the coefficient, the steps and the two bias corrections per tensor -- every double pow of the step
// lives here) and az_adam_multi, a pure stream of 28 B per parameter (p, g, m, v in; p, m, v out).
// One workgroup owns 1024 consecutive elements of ONE tensor (block_desc / first_block as in az_pack_f16_multi), a thread
// four of them.  Nothing here accumulates through atomics: the norm has the same bits on every run.
#include "az_common.h"

#define OPT_BLOCK 256
#define OPT_VEC 4

typedef float opt_f32x4 __attribute__((ext_vector_type(4)));

__device__ __forceinline__ bool opt_aligned16(const AzAdamDesc &d) {
    return ((reinterpret_cast<uintptr_t>(d.param) | reinterpret_cast<uintptr_t>(d.grad) | reinterpret_cast<uintptr_t>(d.exp_avg) |
             reinterpret_cast<uintptr_t>(d.exp_avg_sq)) & 15) == 0;
}

// the sum of x over the workgroup in a FIXED order (xor tree inside a wave, then the waves in index order), in thread 0;
// called by every thread (a barrier inside), blockDim.x == OPT_BLOCK
__device__ __forceinline__ double opt_block_sum(double x) {
    __shared__ double red[OPT_BLOCK / AZ_WAVE];
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) x += __shfl_xor(x, off);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = x;
    __syncthreads();
    double s = red[0];
#pragma unroll
    for (int wv = 1; wv < OPT_BLOCK / AZ_WAVE; ++wv) s += red[wv];
    return s;
}

// ---- K27 -----------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(OPT_BLOCK)
grad_sumsq_multi_kernel(double *__restrict__ partials, const AzAdamDesc *__restrict__ descs, const int *__restrict__ block_desc,
                        const int *__restrict__ first_block) {
    const int di = block_desc[blockIdx.x];
    const AzAdamDesc d = descs[di];  // (block-uniform: scalar loads)
    const long long i = ((long long)(blockIdx.x - first_block[di]) * OPT_BLOCK + threadIdx.x) * OPT_VEC;
    double s = 0.0;
    if (i + OPT_VEC <= d.n && (reinterpret_cast<uintptr_t>(d.grad) & 15) == 0) {
        const opt_f32x4 g = *reinterpret_cast<const opt_f32x4 *>(d.grad + i);  // (read again by K28: a plain load)
        s = ((double)g.x * (double)g.x + (double)g.y * (double)g.y) + ((double)g.z * (double)g.z + (double)g.w * (double)g.w);
    } else {
        for (int e = 0; e < OPT_VEC; ++e)
            if (i + e < d.n) {
                const double g = (double)d.grad[i + e];
                s += g * g;
            }
    }
    s = opt_block_sum(s);
    if (threadIdx.x == 0) partials[blockIdx.x] = s;
}

extern "C" int az_grad_sumsq_multi(double *partials, const AzAdamDesc *descs, const int *block_desc, const int *first_block,
                                   int nd, int nblocks, void *stream) {
    AZ_REQUIRE_PTR(partials); AZ_REQUIRE_PTR(descs); AZ_REQUIRE_PTR(block_desc); AZ_REQUIRE_PTR(first_block);
    AZ_REQUIRE(nd > 0 && nblocks > 0);
    hipLaunchKernelGGL(grad_sumsq_multi_kernel, dim3((unsigned)nblocks), dim3(OPT_BLOCK), 0, az_stream(stream), partials, descs,
                       block_desc, first_block);
    return az_launch_status();
}

// ---- begin ---------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(OPT_BLOCK)
optim_begin_kernel(float *__restrict__ head, float *__restrict__ rec, const AzAdamDesc *__restrict__ descs, int nd,
                   const double *__restrict__ partials, int nblocks_norm, const float *__restrict__ grad_scale,
                   const float *__restrict__ found_inf, double lr, double beta1, double beta2, double max_norm) {
    double s = 0.0;
    for (int b = threadIdx.x; b < nblocks_norm; b += OPT_BLOCK) s += partials[b];
    __shared__ double total;
    s = opt_block_sum(s);
    if (threadIdx.x == 0) total = s;
    __syncthreads();
    const double sum = total;
    const double inv_scale = grad_scale != nullptr ? 1.0 / (double)grad_scale[0] : 1.0;
    const double total_norm = sqrt(sum) * inv_scale;
    const double clip_coef = max_norm >= 0.0 ? fmin(1.0, max_norm / (total_norm + 1e-6)) : 1.0;
    const bool skip = !isfinite(sum) || (found_inf != nullptr && found_inf[0] != 0.f);
    if (threadIdx.x == 0) {
        head[0] = (float)total_norm;
        head[1] = (float)(inv_scale * clip_coef);
        head[2] = skip ? 1.f : 0.f;
        head[3] = (float)clip_coef;
    }
    if (skip) return;
    for (int di = threadIdx.x; di < nd; di += OPT_BLOCK) {
        float *sp = descs[di].step;
        const float step = *sp + 1.f;
        *sp = step;
        rec[2 * di] = (float)(lr / (1.0 - pow(beta1, (double)step)));
        rec[2 * di + 1] = (float)sqrt(1.0 - pow(beta2, (double)step));
    }
}

extern "C" int az_optim_begin(float *head, float *rec, const AzAdamDesc *descs, int nd, const double *partials,
                              int nblocks_norm, const float *grad_scale, const float *found_inf, double lr, double beta1,
                              double beta2, double max_norm, void *stream) {
    AZ_REQUIRE_PTR(head); AZ_REQUIRE_PTR(rec); AZ_REQUIRE_PTR(descs);
    AZ_REQUIRE(nd > 0 && nblocks_norm >= 0);
    if (nblocks_norm > 0) AZ_REQUIRE_PTR(partials);
    AZ_REQUIRE(lr >= 0.0 && beta1 >= 0.0 && beta1 < 1.0 && beta2 >= 0.0 && beta2 < 1.0 && max_norm == max_norm);
    hipLaunchKernelGGL(optim_begin_kernel, dim3(1), dim3(OPT_BLOCK), 0, az_stream(stream), head, rec, descs, nd, partials,
                       nblocks_norm, grad_scale, found_inf, lr, beta1, beta2, max_norm);
    return az_launch_status();
}

// ---- K28 -----------------------------------------------------------------------------------------------------------------
struct OptHyper {
    float one_minus_b1, b2, one_minus_b2, eps, wd, decay;  // decay = 1 - lr * weight_decay (decoupled)
    int decoupled, use_mult;
};

// one element, in the order of torch's _single_tensor_adam
__device__ __forceinline__ void opt_adam(float &p, float g, float &m, float &v, float mult, float step_size, float bc2sqrt,
                                         const OptHyper &h) {
    if (h.use_mult) g *= mult;
    if (h.wd != 0.f) {
        if (h.decoupled) p *= h.decay;
        else g += h.wd * p;
    }
    m += h.one_minus_b1 * (g - m);
    v = h.b2 * v + (h.one_minus_b2 * g) * g;
    p -= (step_size * m) / (sqrtf(v) / bc2sqrt + h.eps);
}

__global__ void __launch_bounds__(OPT_BLOCK)
adam_multi_kernel(const AzAdamDesc *__restrict__ descs, const int *__restrict__ block_desc, const int *__restrict__ first_block,
                  const float *__restrict__ head, const float *__restrict__ rec, OptHyper h) {
    if (head[2] != 0.f) return;  // non-finite gradients, or the caller's found_inf: nothing is written
    const float mult = head[1];
    const int di = block_desc[blockIdx.x];
    const AzAdamDesc d = descs[di];  // (block-uniform: scalar loads, like head and rec)
    const float step_size = rec[2 * di], bc2sqrt = rec[2 * di + 1];
    const long long i = ((long long)(blockIdx.x - first_block[di]) * OPT_BLOCK + threadIdx.x) * OPT_VEC;
    if (i >= d.n) return;
    if (i + OPT_VEC <= d.n && opt_aligned16(d)) {
        const opt_f32x4 g = __builtin_nontemporal_load(reinterpret_cast<const opt_f32x4 *>(d.grad + i));  // read once
        float4 p = *reinterpret_cast<const float4 *>(d.param + i);  // (a struct: its members bind to references)
        float4 m = *reinterpret_cast<const float4 *>(d.exp_avg + i);
        float4 v = *reinterpret_cast<const float4 *>(d.exp_avg_sq + i);
        opt_adam(p.x, g.x, m.x, v.x, mult, step_size, bc2sqrt, h);
        opt_adam(p.y, g.y, m.y, v.y, mult, step_size, bc2sqrt, h);
        opt_adam(p.z, g.z, m.z, v.z, mult, step_size, bc2sqrt, h);
        opt_adam(p.w, g.w, m.w, v.w, mult, step_size, bc2sqrt, h);
        *reinterpret_cast<float4 *>(d.param + i) = p;
        *reinterpret_cast<float4 *>(d.exp_avg + i) = m;
        *reinterpret_cast<float4 *>(d.exp_avg_sq + i) = v;
    } else {
        for (int e = 0; e < OPT_VEC; ++e)
            if (i + e < d.n) {
                float p = d.param[i + e], m = d.exp_avg[i + e], v = d.exp_avg_sq[i + e];
                opt_adam(p, d.grad[i + e], m, v, mult, step_size, bc2sqrt, h);
                d.param[i + e] = p;
                d.exp_avg[i + e] = m;
                d.exp_avg_sq[i + e] = v;
            }
    }
}

extern "C" int az_adam_multi(const AzAdamDesc *descs, const int *block_desc, const int *first_block, int nd, int nblocks,
                             const float *head, const float *rec, double lr, double beta1, double beta2, double eps,
                             double weight_decay, int decoupled, int use_mult, void *stream) {
    AZ_REQUIRE_PTR(descs); AZ_REQUIRE_PTR(block_desc); AZ_REQUIRE_PTR(first_block); AZ_REQUIRE_PTR(head); AZ_REQUIRE_PTR(rec);
    AZ_REQUIRE(nd > 0 && nblocks > 0);
    AZ_REQUIRE(lr >= 0.0 && beta1 >= 0.0 && beta1 < 1.0 && beta2 >= 0.0 && beta2 < 1.0 && eps >= 0.0 && weight_decay >= 0.0);
    OptHyper h;
    h.one_minus_b1 = (float)(1.0 - beta1);
    h.b2 = (float)beta2;
    h.one_minus_b2 = (float)(1.0 - beta2);
    h.eps = (float)eps;
    h.wd = (float)weight_decay;
    h.decay = (float)(1.0 - lr * weight_decay);
    h.decoupled = decoupled != 0;
    h.use_mult = use_mult != 0;
    hipLaunchKernelGGL(adam_multi_kernel, dim3((unsigned)nblocks), dim3(OPT_BLOCK), 0, az_stream(stream), descs, block_desc,
                       first_block, head, rec, h);
    return az_launch_status();
}
