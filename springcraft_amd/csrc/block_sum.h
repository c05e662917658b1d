// The workgroup sum of the conformational-ensemble kernels (superpose.hip, ensemble_pca.hip): a fixed order, no atomics.
#pragma once
#include <hip/hip_runtime.h>

// v[e] <- the sum of v[e] over the workgroup's threads, in every thread: a xor butterfly inside each wavefront (the two
// partners of a level add the same two numbers, so all lanes end with the same bits), then the wavefronts' sums in
// ascending order.  red: NV doubles per wavefront of LDS.  Every thread of the workgroup must call it.
template <int NV>
__device__ __forceinline__ void block_sum(double (&v)[NV], double* red) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nw = blockDim.x >> 6;
#pragma unroll
  for (int e = 0; e < NV; ++e)
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) v[e] += __shfl_xor(v[e], off);
  __syncthreads();   // (the previous sum's readers are done with red)
  if (lane == 0)
#pragma unroll
    for (int e = 0; e < NV; ++e) red[wave * NV + e] = v[e];
  __syncthreads();
#pragma unroll
  for (int e = 0; e < NV; ++e) {
    double s = red[e];
    for (int w = 1; w < nw; ++w) s += red[w * NV + e];
    v[e] = s;
  }
}
