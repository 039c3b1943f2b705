// Block reduction of the loss kernels (K12 az_disp_loss.hip, K16 az_convex_up.hip): N fp64 partial sums per thread,
// wave shuffles, then LDS across the block's waves, and ONE fp64 atomic per block and accumulator.
#pragma once
#include "az_common.h"

// with an atomic per wave the 130 k same-address adds of a 4 x 544 x 960 map
// serialised in L2 and the kernel took 0.79 ms instead of ~15 us
// called by EVERY thread of the workgroup (a barrier inside); blockDim.x == BLOCK
template <int N, int BLOCK>
__device__ __forceinline__ void az_block_sum_f64(double (&v)[N], double *acc) {
    __shared__ double red[BLOCK / 64][N];
#pragma unroll
    for (int k = 0; k < N; ++k) {
        double x = v[k];
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) x += __shfl_xor(x, off);
        if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6][k] = x;
    }
    __syncthreads();
    if (threadIdx.x < N) {
        double x = 0.0;
#pragma unroll
        for (int wv = 0; wv < BLOCK / 64; ++wv) x += red[wv][threadIdx.x];
        if (x != 0.0) atomicAdd(&acc[threadIdx.x], x);
    }
}
