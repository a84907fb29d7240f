// What the resampling routines share (perm.hip: permutation_test, boot.hip: bootstrap): a float64 block product of two
// staged row chunks on the matrix pipe, a one-sided Jacobi SVD in LDS, and the host's checks and batch loop.  Each piece is
// described here once; the two kernels' files say only what they do with it.  Every sum below has a fixed order and there is
// no floating-point atomic, so a resample's bits do not depend on how many resamples a call holds.
//
//   Block product.  A workgroup of 256 threads stages RS_S = 32 rows of two row-major operands in LDS, row stride RS_LW
//                   (padding columns zero), and multiplies A' B with v_mfma_f64_16x16x4f64: A operand block row (= A column)
//                   = lane & 15, sample = lane >> 4; B operand sample = lane >> 4, block column = lane & 15; C/D column =
//                   lane & 15, row = (lane >> 4) + 4 reg.  Wave w owns row tile w % nrt (nrt = row tiles of 16, at most 4)
//                   and, when nrt <= 2, the k-steps 4 / nrt apart from w / nrt on; those groups' accumulators are added in
//                   wave order through LDS at the end (fold_kgroups).  Staging is the caller's: it is what differs.
//   One-sided (Hestenes) Jacobi.  The m x r matrix (r <= m <= RS_MAXP) lies in LDS by columns; the round-robin pairs of
//                   jacobi_dev.h, 8 lanes per pair (Gram entries by an 8-lane butterfly, the rotation of jac_rotation), sweeps
//                   until no pair of a sweep exceeds 4 eps sqrt(a_pp a_qq).  The singular values are the column norms, ranked
//                   descending.  One-sided Jacobi keeps the small singular values to relative accuracy; the Gram route (EVD of
//                   T' T) would cost an absolute eps * sigma_1^2 / sigma_j.  What a non-finite norm means is the caller's.
#pragma once

#include <algorithm>
#include <cstdint>

#include "hip_common.h"
#include "jacobi_dev.h"

namespace ccz {

constexpr int RS_ROWS = CCZ_PERM_ROWS;               // rows per split: the row split is a function of n alone
constexpr int RS_MAXP = CCZ_PERM_MAXP;               // widest view
constexpr int RS_S = 32;                             // rows per staged chunk
constexpr int RS_LW = 80;                            // LDS row stride of a staged chunk (80 % 32 == 16, as krmoment.hip)
constexpr int RS_LDA = RS_MAXP + 1;                  // LDS column stride of the Jacobi matrix
constexpr int RS_SWEEPS = 30;
constexpr int64_t RS_SCRATCH = int64_t(1) << 25;     // doubles of partials per launch (256 MiB)
constexpr int64_t RS_MAXBATCH = 65535;               // gridDim.y

typedef double v4f64 __attribute__((ext_vector_type(4)));

__device__ __forceinline__ double rs_nan() { return __longlong_as_double(0x7ff8000000000000LL); }

__device__ __forceinline__ double sum8(double v) {       // every lane of an aligned group of 8 gets the same bits
  v += __shfl_xor(v, 4, 8);
  v += __shfl_xor(v, 2, 8);
  v += __shfl_xor(v, 1, 8);
  return v;
}
__device__ __forceinline__ double sum4(double v) {
  v += __shfl_xor(v, 2, 4);
  v += __shfl_xor(v, 1, 4);
  return v;
}

// The lanes' places in the block product: row tile rt, k-step group grp of G.
struct mma_lanes {
  int lane, wave, li, lg, nrt, G, rt, grp;
  __device__ __forceinline__ explicit mma_lanes(int nrt_)
      : lane(threadIdx.x & 63), wave(threadIdx.x >> 6), li(lane & 15), lg(lane >> 4), nrt(nrt_), G(4 / nrt_), rt(wave % nrt_),
        grp(wave / nrt_) {}
};

// acc += (this wave's k-steps of the staged chunk As' Bs); upper: only the column tiles on or above the diagonal.  (A runtime
// flag, not a template one: k_boot_moments chooses per workgroup, and two instances of this loop in one kernel cost it 26 VGPRs
// and 1 - 7 % of its time.)
__device__ __forceinline__ void mma_chunk(const double* As, const double* Bs, const mma_lanes& L, bool upper, int nct, v4f64 (&acc)[4]) {
  if (L.grp >= L.G) return;                              // nrt == 3: the fourth wave has no tile
  for (int k4 = 4 * L.grp; k4 < RS_S; k4 += 4 * L.G) {
    const double av = As[(k4 + L.lg) * RS_LW + 16 * L.rt + L.li];
    const double* br = Bs + (k4 + L.lg) * RS_LW + L.li;
#pragma unroll
    for (int ct = 0; ct < 4; ++ct)
      if (ct < nct && (!upper || ct >= L.rt)) acc[ct] = __builtin_amdgcn_mfma_f64_16x16x4f64(av, br[16 * ct], acc[ct], 0, 0, 0);
  }
}

// nrt <= 2: every wave is active; the k-step groups are added in wave order into group 0's acc.  lds: 4096 doubles, free.
__device__ __forceinline__ void fold_kgroups(double* lds, const mma_lanes& L, v4f64 (&acc)[4]) {
  if (L.G == 1) return;
  __syncthreads();
#pragma unroll
  for (int ct = 0; ct < 4; ++ct)
#pragma unroll
    for (int g = 0; g < 4; ++g) lds[((L.wave * 4 + ct) * 4 + g) * 64 + L.lane] = acc[ct][g];
  __syncthreads();
  if (L.grp != 0) return;
#pragma unroll
  for (int ct = 0; ct < 4; ++ct)
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      double s = lds[((L.rt * 4 + ct) * 4 + g) * 64 + L.lane];
      for (int q = 1; q < L.G; ++q) s += lds[(((L.rt + L.nrt * q) * 4 + ct) * 4 + g) * 64 + L.lane];
      acc[ct][g] = s;
    }
}

// Group 0's tiles to the row-major block out (row stride ld); upper as in mma_chunk.
__device__ __forceinline__ void store_tiles(double* __restrict__ out, int ld, const mma_lanes& L, bool upper, int nct, const v4f64 (&acc)[4]) {
  if (L.grp != 0) return;
#pragma unroll
  for (int ct = 0; ct < 4; ++ct) {
    if (ct >= nct || (upper && ct < L.rt)) continue;
#pragma unroll
    for (int g = 0; g < 4; ++g) out[(16 * L.rt + L.lg + 4 * g) * ld + 16 * ct + L.li] = acc[ct][g];
  }
}

// Sweeps over the m x r matrix whose column j is A + j * lda, by all 256 threads; WITH_V: the r x r matrix V (same layout)
// takes the same rotations.  Returns whether a sweep moved nothing within max_sweeps.  The test of a pair is false for NaN: a
// non-finite matrix never "moves", settles at once and is caught by its norms.  moved: one int of LDS.
template <bool WITH_V>
__device__ __forceinline__ bool hestenes_sweeps(double* A, double* V, int lda, int m, int r, int max_sweeps, int* moved) {
  const int tid = threadIdx.x, g8 = tid >> 3, t8 = tid & 7;
  const int re = (r + 1) & ~1, m1 = re - 1, np = re >> 1;
  const double tol = 4.0 * 2.220446049250313e-16;
  bool settled = false;
  for (int sweep = 0; sweep < max_sweeps && !settled; ++sweep) {
    __syncthreads();
    if (tid == 0) *moved = 0;
    for (int round = 0; round < m1; ++round) {
      __syncthreads();
      int p = re, q = re;
      if (g8 < np) pair_of(round, g8, m1, p, q);
      if (p < r && q < r) {
        double* ap = A + p * lda;
        double* aq = A + q * lda;
        double hpp = 0.0, hqq = 0.0, hpq = 0.0;
        for (int i = t8; i < m; i += 8) {
          const double x = ap[i], y = aq[i];
          hpp = fma(x, x, hpp); hqq = fma(y, y, hqq); hpq = fma(x, y, hpq);
        }
        hpp = sum8(hpp); hqq = sum8(hqq); hpq = sum8(hpq);
        if (fabs(hpq) > tol * sqrt(hpp * hqq)) {
          const jac_cs cs = jac_rotation(hpp, hqq, hpq, 1.0 / fmax(fmax(hpp, hqq), fabs(hpq)));
          for (int i = t8; i < m; i += 8) {
            const double x = ap[i], y = aq[i];
            ap[i] = cs.x * x - cs.y * y;
            aq[i] = cs.y * x + cs.x * y;
          }
          if (WITH_V) {
            double* vp = V + p * lda;
            double* vq = V + q * lda;
            for (int i = t8; i < r; i += 8) {
              const double x = vp[i], y = vq[i];
              vp[i] = cs.x * x - cs.y * y;
              vq[i] = cs.y * x + cs.x * y;
            }
          }
          if (t8 == 0) *moved = 1;
        }
      }
    }
    __syncthreads();
    settled = *moved == 0;
  }
  __syncthreads();
  return settled;
}

// put(j, |a_j|^2) for every column j, from one lane; the sum of squares has every lane of the column's 8 in it.
template <class F>
__device__ __forceinline__ void column_norms(const double* A, int lda, int m, int r, F put) {
  const int g8 = threadIdx.x >> 3, t8 = threadIdx.x & 7;
  for (int j = g8; j < r; j += 32) {
    double s = 0.0;
    for (int i = t8; i < m; i += 8) s = fma(A[j * lda + i], A[j * lda + i], s);
    s = sum8(s);
    if (t8 == 0) put(j, s);
  }
}

// The place of nrm[j] among nrm[0 .. r) in descending order (equal values: the lower index first).
__device__ __forceinline__ int rank_desc(const double* nrm, int r, int j) {
  const double v = nrm[j];
  int rank = 0;
  for (int k = 0; k < r; ++k) rank += (nrm[k] > v || (nrm[k] == v && k < j)) ? 1 : 0;
  return rank;
}

// ---- host side
// The checks both entries make, in this order.  counted: "n, p1, p2 and nperm" (extra: the caller's further counts are
// positive); lone: what a NULL draws pointer stands for, e.g. "the identity (perms_dev = NULL) is one permutation".
inline void check_two_views(const char* name, const char* counted, bool extra, bool pointers, const char* lone, const char* count_name,
                            bool draws, int64_t count, int64_t n, int64_t p1, int64_t p2) {
  if (n < 1 || p1 < 1 || p2 < 1 || count < 1 || !extra) fail(CCZ_EINVAL, "%s: %s must be positive", name, counted);
  if (!pointers) fail(CCZ_EINVAL, "%s: null pointer", name);
  if (!draws && count != 1) fail(CCZ_EINVAL, "%s: %s, got %s = %lld", name, lone, count_name, (long long)count);
  if (p1 > RS_MAXP || p2 > RS_MAXP) fail(CCZ_EUNSUP, "%s: views of at most %d columns, got %lld and %lld", name, RS_MAXP, (long long)p1, (long long)p2);
  if (n >= (int64_t(1) << 31)) fail(CCZ_EUNSUP, "%s: fewer than 2^31 rows, got %lld", name, (long long)n);
}

// fn(part, b0, nb, cap) for the items [b0, b0 + nb) of total, at most cap at a time: as many as RS_SCRATCH doubles of partials
// (per_item each, in part) and gridDim.y allow.  A call with more items runs as several launch groups.
template <class F>
void for_batches(ccz_ctx* c, int64_t total, int64_t per_item, F fn) {
  const int64_t cap = std::min(total, std::max<int64_t>(1, std::min<int64_t>(RS_SCRATCH / per_item, RS_MAXBATCH)));
  DBuf part(c, cap * per_item);
  for (int64_t b0 = 0; b0 < total; b0 += cap) fn(part.get(), b0, std::min(cap, total - b0), cap);
}

}  // namespace ccz
