// Permutation null of the two-view singular values: for every permutation pi_b of the rows of view 2 the singular values of
//   T_b = scale * Z_1' Z_2[pi_b]          Z_i (n x p_i, float64, row-major, p_i <= 64): the whitened views
// (cca_zoo_amd/model_selection/_permutation.py; the reference has no counterpart -- the specification is
// tests/perm_restatement.py).  A row permutation of one view leaves both means and both covariances as they are, so the views
// are whitened ONCE and a permutation costs one gathered cross-moment product and one small SVD.
//
//   k_perm_cross     grid (row split, permutation), 256 threads.  A workgroup owns rows [z * CCZ_PERM_ROWS, (z + 1) * CCZ_PERM_ROWS) of
//                    ONE permutation and the whole P1 x P2 product (P_i = p_i rounded up to 16, padding columns zero in LDS).  Per
//                    chunk of 32 rows it stages the rows of Z_1 in order (the chunk is one contiguous block) and the rows
//                    Z_2[pi_b[s]] (each at most 512 contiguous bytes) and multiplies with v_mfma_f64_16x16x4f64: A operand
//                    T row (= Z_1 column) = lane & 15, sample = lane >> 4; B operand sample = lane >> 4, T column = lane & 15;
//                    C/D column = lane & 15, row = (lane >> 4) + 4 reg.  Wave w owns T row tile w % nrt (nrt = P1 / 16) and, when
//                    nrt <= 2, the k-steps 4 / nrt apart from w / nrt on: those waves' accumulators are added in wave order
//                    through LDS at the end.  The partial goes to part[permutation][split][P1][P2].
//   k_perm_fold_svd  grid (permutation), 256 threads.  T_b = scale * (part[b][0] + part[b][1] + ..) in split order into LDS with
//                    the narrower side as columns, then one-sided (Hestenes) Jacobi: the round-robin pairs of jacobi_dev.h, 8
//                    lanes per pair (Gram entries by an 8-lane butterfly, the rotation of jac_rotation), sweeps until no pair
//                    of a sweep exceeds 4 eps sqrt(a_pp a_qq).  The column norms, sorted descending by rank, are sv[b][:].
//                    One-sided Jacobi keeps the small singular values to relative accuracy; the Gram route (EVD of T' T) would
//                    cost an absolute eps * sigma_1^2 / sigma_j.
// The split of the rows is a function of n alone and every sum has a fixed order: no floating-point atomics, and the bits of
// sv[b][:] do not depend on how many permutations a call holds.  A call with more permutations than the scratch budget allows
// runs as several launch pairs.
#include <algorithm>
#include <cstdint>

#include "abi_guard.h"
#include "hip_common.h"
#include "jacobi_dev.h"

namespace ccz {

namespace {

constexpr int PERM_ROWS = CCZ_PERM_ROWS;             // rows per split
constexpr int PERM_MAXP = CCZ_PERM_MAXP;             // widest view
constexpr int PERM_S = 32;                           // rows per staged chunk
constexpr int PERM_LW = 80;                          // LDS row stride of a staged chunk (80 % 32 == 16, as krmoment.hip)
constexpr int PERM_LDA = PERM_MAXP + 1;              // LDS column stride of the Jacobi matrix
constexpr int PERM_SWEEPS = 30;
constexpr int64_t PERM_SCRATCH = int64_t(1) << 25;   // doubles of partials per launch (256 MiB)
constexpr int64_t PERM_MAXBATCH = 65535;             // gridDim.y

typedef double v4f64 __attribute__((ext_vector_type(4)));

__global__ void __launch_bounds__(256) k_perm_cross(const double* __restrict__ Z1, const double* __restrict__ Z2,
                                                    const int* __restrict__ perms, int64_t n, int p1, int p2, int nrt, int nct,
                                                    double* __restrict__ part) {
  __shared__ double lds[2 * PERM_S * PERM_LW];
  double* As = lds;
  double* Bs = lds + PERM_S * PERM_LW;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, li = lane & 15, lg = lane >> 4;
  const int G = 4 / nrt, rt = wave % nrt, grp = wave / nrt;
  const bool active = grp < G;
  const int P1 = 16 * nrt, P2 = 16 * nct;
  const int64_t sb = int64_t(blockIdx.x) * PERM_ROWS;
  const int64_t se = sb + PERM_ROWS < n ? sb + PERM_ROWS : n;
  const int* pi = perms ? perms + int64_t(blockIdx.y) * n : nullptr;
  const int sr = tid >> 4, sc = tid & 15;
  v4f64 acc[4];
#pragma unroll
  for (int ct = 0; ct < 4; ++ct) acc[ct] = v4f64{0.0, 0.0, 0.0, 0.0};
  for (int64_t s0 = sb; s0 < se; s0 += PERM_S) {
    __syncthreads();
    for (int sl = sr; sl < PERM_S; sl += 16) {
      const int64_t s = s0 + sl;
      const bool ok = s < se;
      int64_t g = 0;
      if (ok) {
        g = pi ? int64_t(pi[s]) : s;
        g = g < 0 ? 0 : (g >= n ? n - 1 : g);
      }
      const double* a = Z1 + s * p1;
      const double* b = Z2 + g * p2;
      for (int cc = sc; cc < P1; cc += 16) As[sl * PERM_LW + cc] = (ok && cc < p1) ? a[cc] : 0.0;
      for (int cc = sc; cc < P2; cc += 16) Bs[sl * PERM_LW + cc] = (ok && cc < p2) ? b[cc] : 0.0;
    }
    __syncthreads();
    if (active) {
      for (int k4 = 4 * grp; k4 < PERM_S; k4 += 4 * G) {
        const double av = As[(k4 + lg) * PERM_LW + 16 * rt + li];
        const double* br = Bs + (k4 + lg) * PERM_LW + li;
#pragma unroll
        for (int ct = 0; ct < 4; ++ct)
          if (ct < nct) acc[ct] = __builtin_amdgcn_mfma_f64_16x16x4f64(av, br[16 * ct], acc[ct], 0, 0, 0);
      }
    }
  }
  if (G > 1) {                                           // nrt <= 2: every wave is active; add the k-step groups in wave order
    __syncthreads();
#pragma unroll
    for (int ct = 0; ct < 4; ++ct)
#pragma unroll
      for (int g = 0; g < 4; ++g) lds[((wave * 4 + ct) * 4 + g) * 64 + lane] = acc[ct][g];
    __syncthreads();
    if (grp == 0) {
#pragma unroll
      for (int ct = 0; ct < 4; ++ct)
#pragma unroll
        for (int g = 0; g < 4; ++g) {
          double s = lds[((rt * 4 + ct) * 4 + g) * 64 + lane];
          for (int q = 1; q < G; ++q) s += lds[(((rt + nrt * q) * 4 + ct) * 4 + g) * 64 + lane];
          acc[ct][g] = s;
        }
    }
  }
  if (grp != 0) return;
  double* out = part + (int64_t(blockIdx.y) * gridDim.x + blockIdx.x) * int64_t(P1 * P2);
#pragma unroll
  for (int ct = 0; ct < 4; ++ct) {
    if (ct >= nct) continue;
#pragma unroll
    for (int g = 0; g < 4; ++g) out[(16 * rt + lg + 4 * g) * P2 + 16 * ct + li] = acc[ct][g];
  }
}

__device__ __forceinline__ double sum8(double v) {       // every lane of an aligned group of 8 gets the same bits
  v += __shfl_xor(v, 4, 8);
  v += __shfl_xor(v, 2, 8);
  v += __shfl_xor(v, 1, 8);
  return v;
}

__global__ void __launch_bounds__(256) k_perm_fold_svd(const double* __restrict__ part, int nsplit, int p1, int p2, int P1, int P2,
                                                       double scale, double* __restrict__ sv) {
  __shared__ double A[PERM_MAXP * PERM_LDA];             // column j at A + j * PERM_LDA
  __shared__ double nrm[PERM_MAXP];
  __shared__ int moved;
  const int tid = threadIdx.x, g8 = tid >> 3, t8 = tid & 7;
  const bool tr = p1 < p2;                               // the narrower side of T gives the columns
  const int m = tr ? p2 : p1, r = tr ? p1 : p2;
  const int PP = P1 * P2;
  const double* src = part + int64_t(blockIdx.x) * nsplit * PP;
  for (int e = tid; e < PP; e += 256) {
    const int i = e / P2, j = e - i * P2;
    if (i >= p1 || j >= p2) continue;
    double s = 0.0;
    for (int z = 0; z < nsplit; ++z) s += src[int64_t(z) * PP + e];
    s *= scale;
    if (tr) A[i * PERM_LDA + j] = s; else A[j * PERM_LDA + i] = s;
  }
  const int re = (r + 1) & ~1, m1 = re - 1, np = re >> 1;
  const double tol = 4.0 * 2.220446049250313e-16;
  bool settled = false;
  for (int sweep = 0; sweep < PERM_SWEEPS && !settled; ++sweep) {
    __syncthreads();
    if (tid == 0) moved = 0;
    for (int round = 0; round < m1; ++round) {
      __syncthreads();
      int p = re, q = re;
      if (g8 < np) pair_of(round, g8, m1, p, q);
      if (p < r && q < r) {
        double* ap = A + p * PERM_LDA;
        double* aq = A + q * PERM_LDA;
        double hpp = 0.0, hqq = 0.0, hpq = 0.0;
        for (int i = t8; i < m; i += 8) {
          const double x = ap[i], y = aq[i];
          hpp = fma(x, x, hpp); hqq = fma(y, y, hqq); hpq = fma(x, y, hpq);
        }
        hpp = sum8(hpp); hqq = sum8(hqq); hpq = sum8(hpq);
        if (fabs(hpq) > tol * sqrt(hpp * hqq)) {          // (false for NaN: a non-finite matrix never "moves" and is caught below)
          const jac_cs cs = jac_rotation(hpp, hqq, hpq, 1.0 / fmax(fmax(hpp, hqq), fabs(hpq)));
          for (int i = t8; i < m; i += 8) {
            const double x = ap[i], y = aq[i];
            ap[i] = cs.x * x - cs.y * y;
            aq[i] = cs.y * x + cs.x * y;
          }
          if (t8 == 0) moved = 1;
        }
      }
    }
    __syncthreads();
    settled = moved == 0;
  }
  __syncthreads();
  for (int j = g8; j < r; j += 32) {
    double s = 0.0;
    for (int i = t8; i < m; i += 8) s = fma(A[j * PERM_LDA + i], A[j * PERM_LDA + i], s);
    s = sum8(s);
    if (t8 == 0) nrm[j] = (settled && s == s) ? sqrt(s) : __longlong_as_double(0x7ff8000000000000LL);
  }
  __syncthreads();
  if (tid < r) {
    const double v = nrm[tid];
    int rank = 0;
    for (int k = 0; k < r; ++k) rank += (nrm[k] > v || (nrm[k] == v && k < tid)) ? 1 : 0;
    if (!(v == v)) rank = tid;                             // NaN: every slot of the row is written once
    sv[int64_t(blockIdx.x) * r + rank] = v;
  }
}

void perm_singular_values_impl(ccz_ctx* c, int64_t n, int64_t p1, int64_t p2, const double* Z1, const double* Z2, const int32_t* perms,
                               int64_t nperm, double scale, double* sv) {
  if (n < 1 || p1 < 1 || p2 < 1 || nperm < 1) fail(CCZ_EINVAL, "perm_singular_values: n, p1, p2 and nperm must be positive");
  if (!Z1 || !Z2 || !sv) fail(CCZ_EINVAL, "perm_singular_values: null pointer");
  if (!perms && nperm != 1) fail(CCZ_EINVAL, "perm_singular_values: the identity (perms_dev = NULL) is one permutation, got nperm = %lld", (long long)nperm);
  if (p1 > PERM_MAXP || p2 > PERM_MAXP) fail(CCZ_EUNSUP, "perm_singular_values: views of at most %d columns, got %lld and %lld", PERM_MAXP, (long long)p1, (long long)p2);
  if (n >= (int64_t(1) << 31)) fail(CCZ_EUNSUP, "perm_singular_values: fewer than 2^31 rows, got %lld", (long long)n);
  const int nrt = int(p1 + 15) / 16, nct = int(p2 + 15) / 16, PP = 256 * nrt * nct;
  const int r = int(std::min(p1, p2));
  const int64_t nsplit = (n + PERM_ROWS - 1) / PERM_ROWS;
  const int64_t per = nsplit * PP;
  const int64_t nb_max = std::max<int64_t>(1, std::min<int64_t>(PERM_SCRATCH / per, PERM_MAXBATCH));
  DBuf part(c, std::min(nperm, nb_max) * per);
  for (int64_t b0 = 0; b0 < nperm; b0 += nb_max) {
    const int64_t nb = std::min(nb_max, nperm - b0);
    hipLaunchKernelGGL(k_perm_cross, dim3(unsigned(nsplit), unsigned(nb)), dim3(256), 0, stream(c), Z1, Z2,
                       perms ? perms + b0 * n : nullptr, n, int(p1), int(p2), nrt, nct, part.get());
    CCZ_LAUNCH_CHECK();
    hipLaunchKernelGGL(k_perm_fold_svd, dim3(unsigned(nb)), dim3(256), 0, stream(c), part.get(), int(nsplit), int(p1), int(p2), 16 * nrt,
                       16 * nct, scale, sv + b0 * r);
    CCZ_LAUNCH_CHECK();
  }
}

}  // namespace

}  // namespace ccz

extern "C" {

int ccz_perm_singular_values(ccz_handle h, int64_t n, int64_t p1, int64_t p2, const double* Z1_dev, const double* Z2_dev,
                             const int32_t* perms_dev, int64_t nperm, double scale, double* sv_dev) {
  CCZ_GUARD(h, ccz::perm_singular_values_impl(h, n, p1, p2, Z1_dev, Z2_dev, perms_dev, nperm, scale, sv_dev));
}

}  // extern "C"
