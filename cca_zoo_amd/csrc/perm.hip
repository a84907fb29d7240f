// Permutation null of the two-view singular values: for every permutation pi_b of the rows of view 2 the singular values of
//   T_b = scale * Z_1' Z_2[pi_b]          Z_i (n x p_i, float64, row-major, p_i <= 64): the whitened views
// (cca_zoo_amd/model_selection/_permutation.py; the reference has no counterpart -- the specification is
// tests/perm_restatement.py).  A row permutation of one view leaves both means and both covariances as they are, so the views
// are whitened ONCE and a permutation costs one gathered cross-moment product and one small SVD.  The product, the Jacobi and
// the batch loop are those of resample_dev.h.
//
//   k_perm_cross     grid (row split, permutation), 256 threads.  A workgroup owns rows [z * CCZ_PERM_ROWS, (z + 1) * CCZ_PERM_ROWS) of
//                    ONE permutation and the whole P1 x P2 product (P_i = p_i rounded up to 16).  Per chunk it stages the rows of
//                    Z_1 in order (the chunk is one contiguous block) and the rows Z_2[pi_b[s]] (each at most 512 contiguous
//                    bytes; an index outside [0, n) is clamped, so a bad index cannot fault).  The partial goes to
//                    part[permutation][split][P1][P2].
//   k_perm_fold_svd  grid (permutation), 256 threads.  T_b = scale * (part[b][0] + part[b][1] + ..) in split order into LDS with
//                    the narrower side as columns, then the Jacobi sweeps; sv[b][:] are the ranked column norms.  A matrix
//                    that is not finite or did not settle gives a row of NaN.
#include "abi_guard.h"
#include "resample_dev.h"

namespace ccz {

namespace {

__global__ void __launch_bounds__(256) k_perm_cross(const double* __restrict__ Z1, const double* __restrict__ Z2,
                                                    const int* __restrict__ perms, int64_t n, int p1, int p2, int nrt, int nct,
                                                    double* __restrict__ part) {
  __shared__ double lds[2 * RS_S * RS_LW];
  double* As = lds;
  double* Bs = lds + RS_S * RS_LW;
  const mma_lanes L(nrt);
  const int tid = threadIdx.x;
  const int P1 = 16 * nrt, P2 = 16 * nct;
  const int64_t sb = int64_t(blockIdx.x) * RS_ROWS;
  const int64_t se = sb + RS_ROWS < n ? sb + RS_ROWS : n;
  const int* pi = perms ? perms + int64_t(blockIdx.y) * n : nullptr;
  const int sr = tid >> 4, sc = tid & 15;
  v4f64 acc[4];
#pragma unroll
  for (int ct = 0; ct < 4; ++ct) acc[ct] = v4f64{0.0, 0.0, 0.0, 0.0};
  for (int64_t s0 = sb; s0 < se; s0 += RS_S) {
    __syncthreads();
    for (int sl = sr; sl < RS_S; sl += 16) {
      const int64_t s = s0 + sl;
      const bool ok = s < se;
      int64_t g = 0;
      if (ok) {
        g = pi ? int64_t(pi[s]) : s;
        g = g < 0 ? 0 : (g >= n ? n - 1 : g);
      }
      const double* a = Z1 + s * p1;
      const double* b = Z2 + g * p2;
      for (int cc = sc; cc < P1; cc += 16) As[sl * RS_LW + cc] = (ok && cc < p1) ? a[cc] : 0.0;
      for (int cc = sc; cc < P2; cc += 16) Bs[sl * RS_LW + cc] = (ok && cc < p2) ? b[cc] : 0.0;
    }
    __syncthreads();
    mma_chunk(As, Bs, L, false, nct, acc);
  }
  fold_kgroups(lds, L, acc);
  store_tiles(part + (int64_t(blockIdx.y) * gridDim.x + blockIdx.x) * int64_t(P1 * P2), P2, L, false, nct, acc);
}

__global__ void __launch_bounds__(256) k_perm_fold_svd(const double* __restrict__ part, int nsplit, int p1, int p2, int P1, int P2,
                                                       double scale, double* __restrict__ sv) {
  __shared__ double A[RS_MAXP * RS_LDA];                 // column j at A + j * RS_LDA
  __shared__ double nrm[RS_MAXP];
  __shared__ int moved;
  const int tid = threadIdx.x;
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
    if (tr) A[i * RS_LDA + j] = s; else A[j * RS_LDA + i] = s;
  }
  const bool settled = hestenes_sweeps<false>(A, nullptr, RS_LDA, m, r, RS_SWEEPS, &moved);
  column_norms(A, RS_LDA, m, r, [&](int j, double s) { nrm[j] = (settled && s == s) ? sqrt(s) : rs_nan(); });
  __syncthreads();
  if (tid < r) {
    // One NaN norm makes the whole row NaN, every slot written once.  (With p1 < p2 the columns are the ROWS of T, so a NaN in
    // Z_1 reaches one column only: ranking the others beside it would write one slot twice and leave the last one untouched.)
    bool fine = true;
    for (int k = 0; k < r; ++k) fine = fine && nrm[k] == nrm[k];
    sv[int64_t(blockIdx.x) * r + (fine ? rank_desc(nrm, r, tid) : tid)] = fine ? nrm[tid] : rs_nan();
  }
}

void perm_singular_values_impl(ccz_ctx* c, int64_t n, int64_t p1, int64_t p2, const double* Z1, const double* Z2, const int32_t* perms,
                               int64_t nperm, double scale, double* sv) {
  check_two_views("perm_singular_values", "n, p1, p2 and nperm", true, Z1 && Z2 && sv, "the identity (perms_dev = NULL) is one permutation",
                  "nperm", perms != nullptr, nperm, n, p1, p2);
  const int nrt = int(p1 + 15) / 16, nct = int(p2 + 15) / 16, PP = 256 * nrt * nct;
  const int r = int(std::min(p1, p2));
  const int64_t nsplit = (n + RS_ROWS - 1) / RS_ROWS;
  for_batches(c, nperm, nsplit * PP, [&](double* part, int64_t b0, int64_t nb, int64_t) {
    hipLaunchKernelGGL(k_perm_cross, dim3(unsigned(nsplit), unsigned(nb)), dim3(256), 0, stream(c), Z1, Z2,
                       perms ? perms + b0 * n : nullptr, n, int(p1), int(p2), nrt, nct, part);
    CCZ_LAUNCH_CHECK();
    hipLaunchKernelGGL(k_perm_fold_svd, dim3(unsigned(nb)), dim3(256), 0, stream(c), part, int(nsplit), int(p1), int(p2), 16 * nrt,
                       16 * nct, scale, sv + b0 * r);
    CCZ_LAUNCH_CHECK();
  });
}

}  // namespace

}  // namespace ccz

extern "C" {

int ccz_perm_singular_values(ccz_handle h, int64_t n, int64_t p1, int64_t p2, const double* Z1_dev, const double* Z2_dev,
                             const int32_t* perms_dev, int64_t nperm, double scale, double* sv_dev) {
  CCZ_GUARD(h, ccz::perm_singular_values_impl(h, n, p1, p2, Z1_dev, Z2_dev, perms_dev, nperm, scale, sv_dev));
}

}  // extern "C"
