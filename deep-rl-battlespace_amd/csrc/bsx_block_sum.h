// bsx_block_sum.h -- the sum of one value per thread over a workgroup of NW waves, returned in every thread.
#pragma once

#include <hip/hip_runtime.h>

// The order is fixed and part of the result for a floating-point T: the 64 lanes of a wave by an xor tree (offsets 32, 16, .. 1: every
// lane ends with the same bits), then the NW wave sums in index order, starting from 0.  s_w: NW values of LDS that no other use
// overlaps; the workgroup must reach the call together (one __syncthreads inside).
template <class T, int NW>
__device__ inline T block_sum(T x, T* s_w) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) x += __shfl_xor(x, off);
    if ((threadIdx.x & 63) == 0) s_w[threadIdx.x >> 6] = x;
    __syncthreads();
    T t = 0;
#pragma unroll
    for (int w = 0; w < NW; ++w) t += s_w[w];
    return t;
}
