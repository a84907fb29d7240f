// Row loads of the kernels that read the views where they lie (ey.hip, als.hip, gfa.hip): four consecutive features per lane,
// by 16-byte loads where the alignment allows; the column range of a workgroup that takes one split of a view's columns.
#pragma once

#include <hip/hip_runtime.h>

namespace ccz {

// 16-byte loads of 4 consecutive features are allowed when every row start (and mu) is 16-byte aligned
template <typename T>
__device__ __forceinline__ bool vec_ok(const T* X, int64_t ld, const T* mu) {
  constexpr int64_t V = 16 / sizeof(T);
  return (reinterpret_cast<uintptr_t>(X) % 16 == 0) && (ld % V == 0) && (!mu || reinterpret_cast<uintptr_t>(mu) % 16 == 0);
}

// v[q] = p4[q], q < 4, by 16-byte loads (p4 16-byte aligned)
__device__ __forceinline__ void ld4(const float* p4, float* v) {
  const float4 a = *reinterpret_cast<const float4*>(p4);
  v[0] = a.x; v[1] = a.y; v[2] = a.z; v[3] = a.w;
}
__device__ __forceinline__ void ld4(const double* p4, double* v) {
  const double2 a = *reinterpret_cast<const double2*>(p4), b = *reinterpret_cast<const double2*>(p4 + 2);
  v[0] = a.x; v[1] = a.y; v[2] = b.x; v[3] = b.y;
}

// four consecutive entries starting at f0 (zero beyond p); whole-line loads when `vec` and the four lie inside p
template <typename T>
__device__ __forceinline__ void load4(const T* base, int64_t f0, int64_t p, bool vec, T* v) {
  if (vec && f0 + 3 < p) {
    ld4(base + f0, v);
  } else {
#pragma unroll
    for (int q = 0; q < 4; ++q) v[q] = f0 + q < p ? base[f0 + q] : T(0);
  }
}

// the column range [c0, c1) of split `s` of `cs`, in units of 4 columns so that every split starts on a whole line; `s` enters
// the product in the caller's type (blockIdx.y as it is, or an int), so that a kernel's index arithmetic stays what it was
template <typename Index>
__device__ __forceinline__ void split_range(int64_t p, int cs, Index s, int64_t* c0, int64_t* c1) {
  const int64_t units = (p + 3) / 4, per = (units + cs - 1) / cs;
  *c0 = 4 * per * s;
  *c1 = *c0 + 4 * per < p ? *c0 + 4 * per : p;
}

}  // namespace ccz
