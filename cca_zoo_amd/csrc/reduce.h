// Deterministic sums and maxima of doubles over a 64-lane wave and over a workgroup: the wave by an xor butterfly (offsets
// 32, 16, .. 1), the workgroup by its waves in index order.  Every thread gets the result.
#pragma once

#include <hip/hip_runtime.h>

namespace ccz {

__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}
__device__ __forceinline__ double wave_max(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = fmax(v, __shfl_xor(v, o, 64));
  return v;
}

// over a workgroup of NW waves; sh: NW doubles of LDS
template <int NW>
__device__ __forceinline__ double block_sum(double v, double* sh) {
  v = wave_sum(v);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
  __syncthreads();
  double t = 0.0;
#pragma unroll
  for (int w = 0; w < NW; ++w) t += sh[w];
  return t;
}
template <int NW>
__device__ __forceinline__ double block_max(double v, double* sh) {
  v = wave_max(v);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
  __syncthreads();
  double t = sh[0];
#pragma unroll
  for (int w = 1; w < NW; ++w) t = fmax(t, sh[w]);
  return t;
}

// the sum over a workgroup whose wave count is known only at run time; red: >= blockDim.x / 64 doubles of LDS
__device__ __forceinline__ double block_sum_dyn(double v, double* red) {
  v = wave_sum(v);
  const int wave = threadIdx.x >> 6, nw = (blockDim.x + 63) >> 6;
  __syncthreads();
  if ((threadIdx.x & 63) == 0) red[wave] = v;
  __syncthreads();
  double t = 0.0;
  for (int i = 0; i < nw; ++i) t += red[i];
  return t;
}

}  // namespace ccz
