// CP-ALS of a dense float64 tensor in HBM: the factor step of TCCA / KTCCA, whole iterations on the device.
//
// Reference: cca_zoo/linear/_tcca.py:111-117, cca_zoo/nonparametric/_ktcca.py:130-136 call tensorly's parafac with its defaults
// (init="svd", n_iter_max=100, tol=1e-8, no normalisation, stop on the absolute change of the reconstruction error).  tensorly is
// not a dependency here: the algorithm is written out (include/ccz.h states it; tests/tcca_fit_restatement.py is its NumPy form).
// The tensor M is row-major, the last mode's index fastest (ccz_kr_moment's layout), order V = 2..8, prod d_i <= 2^24, rank
// k <= min(32, min d_i).  unfold(M, m) = moveaxis(M, m, 0).reshape(d_m, J_m), J_m = prod_{i != m} d_i.
//
// Setup (ccz_cp_setup; may wait for the host):
//   k_cp_unfold             U_m = unfold(M, m) for m >= 1, once (mode 0's unfolding is M itself): no kernel of an iteration
//                           rewrites or re-lays the tensor, every mode update reads its unfolding exactly once
//   k_cp_sumsq, k_cp_start  ||M||_F^2 by per-workgroup partials folded in index order; the status word
//   init                    the k leading left singular vectors of U_m from the symmetric EVD (syev_full) of the smaller of
//                           U_m U_m' (d_m x d_m: its eigenvectors) and U_m' U_m (J_m x J_m: A_m = U_m V, columns normalised)
//   k_cp_ugram, k_cp_uv     that Gram and that product: 16 x 16 output tiles, the contraction axis split into partials that
//                           k_cp_fold adds in split order (the library's general GEMM splits deep products with atomics)
//   k_cp_colfix             per column: optional normalisation, then the sign that makes the entry of largest magnitude positive
//   k_cp_gram               A_m' A_m (k x k) of every factor
// One iteration, for m = 0 .. V-1 (Gauss-Seidel):
//   k_cp_mttkrp<KT>         G = U_m khatri_rao(A_i, i != m)   (d_m x k).  grid (row tiles, 1, splits of J_m), 256 threads; a
//                           workgroup owns 64 rows (16 per wave) and all k columns.  Per chunk of 32 contraction indices it stages
//                           64 x 32 of U_m and the 32 x k Khatri-Rao rows (a product of V - 1 factor entries each, formed once per
//                           chunk, never in HBM).  k > 4: v_mfma_f64_16x16x4f64 (lane maps as in krmoment.hip: A operand row =
//                           lane & 15, k = lane >> 4; B operand k = lane >> 4, column = lane & 15; C/D column = lane & 15, row =
//                           (lane >> 4) + 4 reg), KT = 1 or 2 column tiles; k <= 4: plain FMAs, one thread per (row, column).
//                           Row, column and contraction tails are zero-filled in LDS.  This is ccz_kr_apply's contraction with
//                           H_i = A_i' and k in the place of the samples; k_kr_apply is not reused because it tiles 64 samples per
//                           workgroup (k <= 32 would idle half of every tile) and copies the tensor into its unfolding per call.
//   k_cp_fold               when the row tiles alone do not fill the chip J_m is split: every split writes its own
//                           [split][d_m][k] partial and the fold adds them in split order (no floating-point atomics)
//   k_cp_update             one workgroup: P = Hadamard product of the other factors' Grams, P^-1 by Gauss-Jordan with partial
//                           pivoting in LDS (a zero or non-finite pivot: status "singular", the fit stops), A_m = G P^-1, the new
//                           Gram of A_m.  After the last mode also F2 = sum of the Hadamard product of all Grams, ip = sum G o A_m,
//                           e_t = sqrt|normM^2 + F2 - 2 ip| / normM, the trace, the stop test and the status word.
// Every kernel of an iteration reads the status word first and returns at once after the stop.  All sums run in a fixed order:
// two fits give the same bits, whatever the chunk length.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <vector>

#include "hip_common.h"
#include "abi_guard.h"
#include "fit_driver.h"
#include "reduce.h"

namespace ccz {

namespace {

constexpr int CP_MAXV = 8;                            // modes per tensor
constexpr int CP_MAXK = 32;                           // rank; also the leading dimension of every k x k matrix in HBM
constexpr int CP_KK = CP_MAXK * CP_MAXK;
constexpr int CP_LD = CP_MAXK + 1;                    // LDS row stride of a k x k matrix (doubles)
constexpr int CP_PT = 1024;                           // threads of the one-workgroup kernels: one per k x k entry
constexpr int64_t CP_MAXPROD = int64_t(1) << 24;      // most tensor entries
constexpr int CP_PLAIN_K = 4;                         // rank up to which the MTTKRP runs on plain FMAs
constexpr int CP_TR = 64;                             // k_cp_mttkrp: rows per workgroup
constexpr int CP_JC = 32;                             // k_cp_mttkrp: contraction indices per staged chunk
constexpr int CP_UW = 36;                             // LDS row stride of the staged unfolding (36 % 32 == 4: the 16 rows x 4 indices of an A operand on distinct slots)
constexpr int CP_MAXSPLIT = 64;                       // most splits of the contraction axis
constexpr int CP_NG = 256;                            // workgroups of k_cp_sumsq

constexpr int CP_RUNNING = 0, CP_TOL = 1, CP_MAXITER = 2, CP_SINGULAR = 3;   // CpStatus::reason (include/ccz.h: CCZ_CP_*)

typedef double v4f64 __attribute__((ext_vector_type(4)));

struct CpStatus {
  double err;                      // e_t of the last finished iteration
  double dec;                      // |e_{t-1} - e_t| of the last finished iteration (0 after the first)
  long long iters;                 // iterations done
  int stopped;
  int reason;
};

// the device buffers and shapes of one fit
struct CpBuf {
  const double* U[CP_MAXV];        // unfold(M, m): d_m x J_m row-major (mode 0: the tensor itself)
  double* A;                       // the factors back to back: A_m (d_m x K) at aoff[m]
  double* gram;                    // V x KK: A_m' A_m
  double* G;                       // dmax x K: the MTTKRP of the mode being updated
  double* part;                    // split partials of G
  double* trace;                   // max_iter doubles: e_t
  double* norm2;                   // ||M||_F^2
  double* npart;                   // CP_NG partial sums of squares
  int64_t aoff[CP_MAXV];
  int d[CP_MAXV];
  int J[CP_MAXV];
  int V, K, max_iter;
  double tol;
};

// ---- U_m = unfold(M, m): (outer, d_m, inner) -> (d_m, outer, inner) ------------------------------------------------------
__global__ void __launch_bounds__(256) k_cp_unfold(const double* __restrict__ T, int64_t total, int dm, int inner, int64_t J,
                                                   double* __restrict__ U) {
  const int64_t e = int64_t(blockIdx.x) * 256 + threadIdx.x;
  if (e >= total) return;
  const int64_t a = e / J, j = e % J, hi = j / inner, lo = j % inner;
  U[e] = T[(hi * dm + a) * inner + lo];
}

// ---- ||M||_F^2: per-workgroup partials, folded in index order by k_cp_start -------------------------------------------------
__global__ void __launch_bounds__(256) k_cp_sumsq(const double* __restrict__ T, int64_t total, double* __restrict__ npart) {
  __shared__ double red[4];
  double s = 0.0;
  for (int64_t e = int64_t(blockIdx.x) * 256 + threadIdx.x; e < total; e += int64_t(CP_NG) * 256) s += T[e] * T[e];
  s = block_sum<4>(s, red);
  if (threadIdx.x == 0) npart[blockIdx.x] = s;
}

// the status word of a new fit; fold_norm: also ||M||_F^2 from the partials
__global__ void k_cp_start(CpBuf B, int fold_norm, CpStatus* st) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  if (fold_norm) {
    double s = 0.0;
    for (int g = 0; g < CP_NG; ++g) s += B.npart[g];
    *B.norm2 = s;
  }
  st->err = 0.0; st->dec = 0.0; st->iters = 0; st->stopped = 0; st->reason = CP_RUNNING;
}

// ---- setup products with a fixed order of summation -----------------------------------------------------------------------
// C (R x R) = X X' over the contraction axis of length L, X(p, t) = TRANS ? U[t, p] : U[p, t] (U has row stride ldu).  grid
// (R / 16, R / 16, splits); split z writes its own R x R partial.
template <bool TRANS>
__global__ void __launch_bounds__(256) k_cp_ugram(const double* __restrict__ U, int64_t ldu, int R, int L, int lps, double* __restrict__ part) {
  __shared__ double Xp[16 * 33], Xq[16 * 33];
  const int tid = threadIdx.x, p0 = int(blockIdx.x) * 16, q0 = int(blockIdx.y) * 16;
  const int tb = int(blockIdx.z) * lps, te = min(L, tb + lps);
  const int pi = tid >> 4, qi = tid & 15;
  double acc = 0.0;
  for (int t0 = tb; t0 < te; t0 += 32) {
    __syncthreads();
    for (int e = tid; e < 512; e += 256) {
      // TRANS: consecutive threads read consecutive p (one row of U); else consecutive t (one row of U)
      const int i = TRANS ? (e & 15) : (e >> 5), tt = TRANS ? (e >> 4) : (e & 31);
      const int t = t0 + tt;
      const bool in = t < te;
      const int p = p0 + i, q = q0 + i;
      Xp[i * 33 + tt] = (in && p < R) ? (TRANS ? U[int64_t(t) * ldu + p] : U[int64_t(p) * ldu + t]) : 0.0;
      Xq[i * 33 + tt] = (in && q < R) ? (TRANS ? U[int64_t(t) * ldu + q] : U[int64_t(q) * ldu + t]) : 0.0;
    }
    __syncthreads();
#pragma unroll 8
    for (int tt = 0; tt < 32; ++tt) acc += Xp[pi * 33 + tt] * Xq[qi * 33 + tt];
  }
  const int p = p0 + pi, q = q0 + qi;
  if (p < R && q < R) part[int64_t(blockIdx.z) * R * R + int64_t(p) * R + q] = acc;
}

// A (d x K) = U (d x J) V' with V (K x J) the leading rows of the eigenvector matrix: one thread per entry, in index order
__global__ void __launch_bounds__(256) k_cp_uv(const double* __restrict__ U, const double* __restrict__ Vr, int64_t d, int J, int K,
                                               double* __restrict__ A) {
  const int64_t e = int64_t(blockIdx.x) * 256 + threadIdx.x;
  if (e >= d * K) return;
  const int64_t a = e / K;
  const int r = int(e % K);
  double s = 0.0;
  for (int j = 0; j < J; ++j) s += U[a * J + j] * Vr[int64_t(r) * J + j];
  A[e] = s;
}

// ---- per column of A (d x K): optional normalisation, then the sign that makes its entry of largest magnitude positive ------
// (the first such entry on a tie, as np.argmax)
__global__ void __launch_bounds__(64) k_cp_colfix(double* __restrict__ A, int d, int K, int normalise) {
  const int r = threadIdx.x;
  if (r >= K) return;
  double ss = 0.0, best = -1.0, bv = 0.0;
  for (int a = 0; a < d; ++a) {
    const double v = A[int64_t(a) * K + r];
    ss += v * v;
    if (fabs(v) > best) { best = fabs(v); bv = v; }
  }
  double f = bv < 0.0 ? -1.0 : 1.0;
  if (normalise) f /= sqrt(ss);
  for (int a = 0; a < d; ++a) A[int64_t(a) * K + r] *= f;
}

// Gram of a factor: thread (r, s) of a CP_PT workgroup sums A[a, r] A[a, s] over the rows in order
__device__ __forceinline__ double cp_gram_entry(const double* A, int d, int K, int r, int s) {
  double g = 0.0;
  if (r < K && s < K)
    for (int a = 0; a < d; ++a) g += A[int64_t(a) * K + r] * A[int64_t(a) * K + s];
  return g;
}

__global__ void __launch_bounds__(CP_PT) k_cp_gram(CpBuf B) {
  const int m = blockIdx.x, r = threadIdx.x >> 5, s = threadIdx.x & 31;
  B.gram[m * CP_KK + r * CP_MAXK + s] = cp_gram_entry(B.A + B.aoff[m], B.d[m], B.K, r, s);
}

// ---- G = U_m khatri_rao(A_i, i != m) ------------------------------------------------------------------------------------
template <int KT>   // 0: plain FMAs (K <= 4); 1, 2: that many 16-column MFMA tiles
__global__ void __launch_bounds__(256) k_cp_mttkrp(CpBuf B, int m, int jps, double* __restrict__ dst, const CpStatus* st) {
  if (fit_stopped(st)) return;
  constexpr int KW = KT == 0 ? CP_PLAIN_K : 16 * KT;    // staged Khatri-Rao columns
  constexpr int KS = KT == 2 ? 48 : KW;                 // their LDS row stride (48 % 32 == 16: two rows of a half wave on disjoint slots)
  __shared__ double Us[CP_TR * CP_UW];
  __shared__ double Ks[CP_JC * KS];
  const int tid = threadIdx.x;
  const int d = B.d[m], J = B.J[m], K = B.K;
  const double* __restrict__ U = B.U[m];
  const int r0 = int(blockIdx.x) * CP_TR;
  const int jb = int(blockIdx.z) * jps, je = min(J, jb + jps);
  v4f64 acc[KT == 0 ? 1 : KT];
#pragma unroll
  for (int ct = 0; ct < (KT == 0 ? 1 : KT); ++ct) acc[ct] = v4f64{0.0, 0.0, 0.0, 0.0};
  for (int j0 = jb; j0 < je; j0 += CP_JC) {
    __syncthreads();
    {
      const int jj = tid & 31, j = j0 + jj;
      for (int row = tid >> 5; row < CP_TR; row += 8) {
        const int a = r0 + row;
        Us[row * CP_UW + jj] = (a < d && j < je) ? U[int64_t(a) * J + j] : 0.0;
      }
    }
    {
      const int jj = tid >> 3, j = j0 + jj;
      int ix[CP_MAXV];
      int rem = j < je ? j : 0;
#pragma unroll
      for (int i = CP_MAXV - 1; i >= 0; --i) {
        ix[i] = 0;
        if (i < B.V && i != m) { ix[i] = rem % B.d[i]; rem /= B.d[i]; }
      }
      for (int r = tid & 7; r < KW; r += 8) {
        double v = 0.0;
        if (j < je && r < K) {
          v = 1.0;
#pragma unroll
          for (int i = 0; i < CP_MAXV; ++i)
            if (i < B.V && i != m) v *= B.A[B.aoff[i] + int64_t(ix[i]) * K + r];
        }
        Ks[jj * KS + r] = v;
      }
    }
    __syncthreads();
    if constexpr (KT == 0) {
      const int row = tid >> 2, r = tid & 3;
      double s = acc[0][0];
#pragma unroll 8
      for (int jj = 0; jj < CP_JC; ++jj) s += Us[row * CP_UW + jj] * Ks[jj * KS + r];
      acc[0][0] = s;
    } else {
      const int lane = tid & 63, wave = tid >> 6, li = lane & 15, lg = lane >> 4;
      const double* ar = Us + (16 * wave + li) * CP_UW + lg;
      const double* br = Ks + lg * KS + li;
#pragma unroll
      for (int k4 = 0; k4 < CP_JC; k4 += 4) {
        const double av = ar[k4];
#pragma unroll
        for (int ct = 0; ct < KT; ++ct) acc[ct] = __builtin_amdgcn_mfma_f64_16x16x4f64(av, br[k4 * KS + 16 * ct], acc[ct], 0, 0, 0);
      }
    }
  }
  double* out = dst + int64_t(blockIdx.z) * d * K;
  if constexpr (KT == 0) {
    const int a = r0 + (tid >> 2), r = tid & 3;
    if (a < d && r < K) out[int64_t(a) * K + r] = acc[0][0];
  } else {
    const int lane = tid & 63, wave = tid >> 6, li = lane & 15, lg = lane >> 4;
#pragma unroll
    for (int ct = 0; ct < KT; ++ct) {
      const int col = 16 * ct + li;
      if (col >= K) continue;
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        const int a = r0 + 16 * wave + lg + 4 * g;
        if (a < d) out[int64_t(a) * K + col] = acc[ct][g];
      }
    }
  }
}

// ---- G = part[0] + part[1] + .. in split order -----------------------------------------------------------------------------
__global__ void __launch_bounds__(256) k_cp_fold(const double* __restrict__ part, int split, int64_t total, double* __restrict__ G,
                                                 const CpStatus* st) {
  if (st && fit_stopped(st)) return;      // st == null: a setup product
  const int64_t e = int64_t(blockIdx.x) * 256 + threadIdx.x;
  if (e >= total) return;
  double s = 0.0;
  for (int z = 0; z < split; ++z) s += part[int64_t(z) * total + e];
  G[e] = s;
}

// ---- the update of mode m: P, its inverse, A_m = G P^-1, the Gram of A_m; after the last mode the error and the stop -----------
__global__ void __launch_bounds__(CP_PT) k_cp_update(CpBuf B, int m, int last, CpStatus* st) {
  if (fit_stopped(st)) return;
  __shared__ double Pm[CP_MAXK * CP_LD], Iv[CP_MAXK * CP_LD], red[16];
  __shared__ int piv, bad;
  const int t = threadIdx.x, r = t >> 5, s = t & 31;
  const int K = B.K, d = B.d[m];
  double p = (r == s) ? 1.0 : 0.0;
  if (r < K && s < K) {
    p = 1.0;
    for (int i = 0; i < B.V; ++i)
      if (i != m) p *= B.gram[i * CP_KK + r * CP_MAXK + s];
  }
  const double p_others = p;
  Pm[r * CP_LD + s] = p;
  Iv[r * CP_LD + s] = (r == s) ? 1.0 : 0.0;
  if (t == 0) bad = 0;
  __syncthreads();
  for (int c = 0; c < K; ++c) {
    if (t == 0) {
      int best = c;
      double bv = fabs(Pm[c * CP_LD + c]);
      for (int q = c + 1; q < K; ++q) {
        const double v = fabs(Pm[q * CP_LD + c]);
        if (v > bv || (v != v)) { bv = v; best = q; }
      }
      piv = best;
      if (!(bv > 0.0) || !isfinite(bv)) bad = 1;
    }
    __syncthreads();
    if (bad) break;
    const int pr = piv;
    if (pr != c && r == c) {   // the 32 threads of row c swap rows c and pr of both matrices
      double x = Pm[c * CP_LD + s]; Pm[c * CP_LD + s] = Pm[pr * CP_LD + s]; Pm[pr * CP_LD + s] = x;
      x = Iv[c * CP_LD + s]; Iv[c * CP_LD + s] = Iv[pr * CP_LD + s]; Iv[pr * CP_LD + s] = x;
    }
    __syncthreads();
    const double f = (r != c && r < K) ? Pm[r * CP_LD + c] / Pm[c * CP_LD + c] : 0.0;
    __syncthreads();
    if (r != c && r < K) {
      Pm[r * CP_LD + s] -= f * Pm[c * CP_LD + s];
      Iv[r * CP_LD + s] -= f * Iv[c * CP_LD + s];
    }
    __syncthreads();
  }
  if (bad) {
    if (t == 0) { st->stopped = 1; st->reason = CP_SINGULAR; }
    return;
  }
  if (r < K) Iv[r * CP_LD + s] /= Pm[r * CP_LD + r];
  __syncthreads();
  double* __restrict__ Am = B.A + B.aoff[m];
  const int64_t total = int64_t(d) * K;
  double ip = 0.0;
  for (int64_t e = t; e < total; e += CP_PT) {
    const int64_t a = e / K;
    const int col = int(e % K);
    double v = 0.0;
    for (int q = 0; q < K; ++q) v += B.G[a * K + q] * Iv[q * CP_LD + col];
    Am[e] = v;
    ip += B.G[e] * v;
  }
  __syncthreads();   // A_m, written above, is read below by other threads of this workgroup
  const double g = cp_gram_entry(Am, d, K, r, s);
  B.gram[m * CP_KK + r * CP_MAXK + s] = g;
  if (!last) return;
  const double f2 = block_sum<16>((r < K && s < K) ? p_others * g : 0.0, red);
  ip = block_sum<16>(ip, red);
  if (t == 0) {
    const double n2 = *B.norm2;
    const double e = sqrt(fabs(n2 + f2 - 2.0 * ip)) / sqrt(n2);
    const long long it = st->iters;
    B.trace[it] = e;
    const double dec = it >= 1 ? fabs(st->err - e) : 0.0;
    st->err = e;
    st->dec = dec;
    st->iters = it + 1;
    if (it >= 1 && dec < B.tol) { st->stopped = 1; st->reason = CP_TOL; }
    else if (it + 1 >= B.max_iter) { st->stopped = 1; st->reason = CP_MAXITER; }
  }
}

// ---- host driver ----------------------------------------------------------------------------------------------------
struct CpState : FitState<CpStatus> {
  CpBuf B;
  int64_t prod = 0, atot = 0;
  int split[CP_MAXV], jps[CP_MAXV];
  bool ready = false;
};

void launch_mttkrp(ccz_ctx* c, const CpState& S, int m, double* dst) {
  const CpBuf& B = S.B;
  const dim3 grid(unsigned((B.d[m] + CP_TR - 1) / CP_TR), 1, unsigned(S.split[m]));
  if (B.K <= CP_PLAIN_K)
    hipLaunchKernelGGL((k_cp_mttkrp<0>), grid, dim3(256), 0, stream(c), B, m, S.jps[m], dst, S.drv.dev);
  else if (B.K <= 16)
    hipLaunchKernelGGL((k_cp_mttkrp<1>), grid, dim3(256), 0, stream(c), B, m, S.jps[m], dst, S.drv.dev);
  else
    hipLaunchKernelGGL((k_cp_mttkrp<2>), grid, dim3(256), 0, stream(c), B, m, S.jps[m], dst, S.drv.dev);
  CCZ_LAUNCH_CHECK();
}

void enqueue_iteration(ccz_ctx* c, const CpState& S) {
  const CpBuf& B = S.B;
  for (int m = 0; m < B.V; ++m) {
    if (S.split[m] == 1) {
      launch_mttkrp(c, S, m, B.G);
    } else {
      launch_mttkrp(c, S, m, B.part);
      const int64_t total = int64_t(B.d[m]) * B.K;
      hipLaunchKernelGGL(k_cp_fold, dim3(unsigned((total + 255) / 256)), dim3(256), 0, stream(c), B.part, S.split[m], total, B.G, S.drv.dev);
      CCZ_LAUNCH_CHECK();
    }
    hipLaunchKernelGGL(k_cp_update, dim3(1), dim3(CP_PT), 0, stream(c), B, m, m == B.V - 1 ? 1 : 0, S.drv.dev);
    CCZ_LAUNCH_CHECK();
  }
}

CpState* cp_create(ccz_ctx* c, int V, const int64_t* dims, int64_t k, double tol, int64_t max_iter, int64_t chunk) {
  if (V < 2 || V > CP_MAXV) fail(CCZ_EUNSUP, "cp: tensors of order 2 to %d are supported, got %d", CP_MAXV, V);
  if (k < 1 || k > CP_MAXK) fail(CCZ_EUNSUP, "cp: ranks 1 to %d are supported, got %lld", CP_MAXK, (long long)k);
  if (!dims || max_iter < 1 || max_iter > (int64_t(1) << 20) || chunk < 1 || !(tol >= 0.0)) fail(CCZ_EINVAL, "cp: bad argument");
  check_no_empty_view("cp", V, dims);
  int64_t prod = 1;
  for (int i = 0; i < V; ++i) {
    if (dims[i] > CP_MAXPROD || (prod *= dims[i]) > CP_MAXPROD) fail(CCZ_EUNSUP, "cp: the tensor has more than 2^24 entries");
  }
  for (int i = 0; i < V; ++i)
    if (k > dims[i]) fail(CCZ_EINVAL, "cp: rank %lld exceeds the width %lld of mode %d", (long long)k, (long long)dims[i], i);
  return new_state<CpState>(c, [&](CpState& S) {
    S.dtype = CCZ_F64; S.M = V; S.chunk = chunk; S.prod = prod;
    S.p.assign(dims, dims + V);
    CpBuf& B = S.B;
    memset(&B, 0, sizeof(B));
    B.V = V; B.K = int(k); B.max_iter = int(max_iter); B.tol = tol;
    const int64_t want = 2 * int64_t(impl(c)->props.multiProcessorCount);
    int64_t dmax = 0, pmax = 0;
    for (int m = 0; m < V; ++m) {
      B.d[m] = int(dims[m]);
      B.J[m] = int(prod / dims[m]);
      B.aoff[m] = S.atot;
      S.atot += dims[m] * k;
      dmax = std::max(dmax, dims[m]);
      // splits of the contraction axis so that row tiles x splits fills the chip
      const int64_t tiles = (dims[m] + CP_TR - 1) / CP_TR, chunks = (int64_t(B.J[m]) + CP_JC - 1) / CP_JC;
      int64_t split = tiles >= want ? 1 : std::max<int64_t>(1, std::min<int64_t>({(want + tiles - 1) / tiles, chunks, CP_MAXSPLIT}));
      S.jps[m] = int((chunks + split - 1) / split * CP_JC);
      S.split[m] = (B.J[m] + S.jps[m] - 1) / S.jps[m];
      if (S.split[m] > 1) pmax = std::max(pmax, int64_t(S.split[m]) * dims[m] * k);
    }
    B.A = S.get(c, size_t(S.atot));
    B.gram = S.get(c, size_t(V) * CP_KK);
    B.G = S.get(c, size_t(dmax) * k);
    B.part = S.get(c, size_t(pmax));
    B.trace = S.get(c, size_t(max_iter));
    B.norm2 = S.get(c, 1);
    B.npart = S.get(c, CP_NG);
    for (int m = 1; m < V; ++m) B.U[m] = S.get(c, size_t(prod));
    S.drv.create(c);
  });
}

// C (R x R) = U U' (!trans: R = d, contraction over J) or U' U (trans: R = J, contraction over d); U is d x J
void cp_ugram(ccz_ctx* c, const double* U, int64_t d, int64_t J, bool trans, double* C) {
  const int R = int(trans ? J : d), L = int(trans ? d : J);
  const int64_t rt = (R + 15) / 16, tiles = rt * rt, chunks = (L + 31) / 32;
  const int64_t want = 2 * int64_t(impl(c)->props.multiProcessorCount);
  int64_t split = tiles >= want ? 1 : std::max<int64_t>(1, std::min<int64_t>({(want + tiles - 1) / tiles, chunks, CP_MAXSPLIT}));
  const int lps = int((chunks + split - 1) / split * 32);
  split = (L + lps - 1) / lps;
  DBuf part;
  if (split > 1) part = DBuf(c, split * int64_t(R) * R);
  double* dst = split > 1 ? part.get() : C;
  const dim3 grid{unsigned(rt), unsigned(rt), unsigned(split)};
  if (trans)
    hipLaunchKernelGGL((k_cp_ugram<true>), grid, dim3(256), 0, stream(c), U, J, R, L, lps, dst);
  else
    hipLaunchKernelGGL((k_cp_ugram<false>), grid, dim3(256), 0, stream(c), U, J, R, L, lps, dst);
  CCZ_LAUNCH_CHECK();
  if (split > 1) {
    const int64_t total = int64_t(R) * R;
    hipLaunchKernelGGL(k_cp_fold, dim3(unsigned((total + 255) / 256)), dim3(256), 0, stream(c), part.get(), int(split), total, C,
                       static_cast<const CpStatus*>(nullptr));
    CCZ_LAUNCH_CHECK();
  }
}

// the k leading left singular vectors of U (d x J) into A (d x K), signs fixed
void cp_init_mode(ccz_ctx* c, const double* U, int64_t d, int64_t J, int K, double* A) {
  std::vector<double> w;
  if (d == 1) {
    fill2d(c, 1, 1, A, 1, 1.0);
    return;
  }
  if (d <= J) {
    DBuf Gm(c, d * d), Vr(c, d * d);
    cp_ugram(c, U, d, J, false, Gm);
    syev_full(c, Gm, d, w, Vr, d);
    transpose(c, K, d, Vr, d, A, K);
    hipLaunchKernelGGL(k_cp_colfix, dim3(1), dim3(64), 0, stream(c), A, int(d), K, 0);
  } else {
    DBuf Vr(c, J * J);
    if (J == 1) {
      fill2d(c, 1, 1, Vr, 1, 1.0);
    } else {
      DBuf Gm(c, J * J);
      cp_ugram(c, U, d, J, true, Gm);
      syev_full(c, Gm, J, w, Vr, J);
    }
    hipLaunchKernelGGL(k_cp_uv, dim3(unsigned((d * K + 255) / 256)), dim3(256), 0, stream(c), U, Vr.get(), d, int(J), K, A);
    CCZ_LAUNCH_CHECK();
    hipLaunchKernelGGL(k_cp_colfix, dim3(1), dim3(64), 0, stream(c), A, int(d), K, 1);
  }
  CCZ_LAUNCH_CHECK();
}

void cp_grams_and_start(ccz_ctx* c, CpState& S, bool fold_norm) {
  hipLaunchKernelGGL(k_cp_gram, dim3(S.B.V), dim3(CP_PT), 0, stream(c), S.B);
  CCZ_LAUNCH_CHECK();
  hipLaunchKernelGGL(k_cp_start, dim3(1), dim3(64), 0, stream(c), S.B, fold_norm ? 1 : 0, S.drv.dev);
  CCZ_LAUNCH_CHECK();
}

void cp_setup(ccz_ctx* c, CpState& S, const double* M) {
  CpBuf& B = S.B;
  B.U[0] = M;
  for (int m = 1; m < B.V; ++m) {
    int64_t inner = 1;
    for (int i = m + 1; i < B.V; ++i) inner *= B.d[i];
    hipLaunchKernelGGL(k_cp_unfold, dim3(unsigned((S.prod + 255) / 256)), dim3(256), 0, stream(c), M, S.prod, B.d[m], int(inner),
                       int64_t(B.J[m]), const_cast<double*>(B.U[m]));
    CCZ_LAUNCH_CHECK();
  }
  hipLaunchKernelGGL(k_cp_sumsq, dim3(CP_NG), dim3(256), 0, stream(c), M, S.prod, B.npart);
  CCZ_LAUNCH_CHECK();
  for (int m = 0; m < B.V; ++m) cp_init_mode(c, B.U[m], B.d[m], B.J[m], B.K, B.A + B.aoff[m]);
  cp_grams_and_start(c, S, true);
}

CpStatus read_status(ccz_ctx* c, const CpState& S) {
  CpStatus st;
  d2h(c, &st, S.drv.dev, sizeof(st));
  return st;
}

}  // namespace
}  // namespace ccz

extern "C" {

int ccz_cp_create(ccz_handle h, int order, const int64_t* dims, int64_t k, double tol, int64_t max_iter, int64_t chunk_iters,
                  void** state_out) {
  CCZ_GUARD(h, {
    if (!state_out) ccz::fail(CCZ_EINVAL, "null argument");
    *state_out = nullptr;
    *state_out = ccz::cp_create(h, order, dims, k, tol, max_iter, chunk_iters);
  })
}

int ccz_cp_destroy(ccz_handle h, void* state) {
  CCZ_GUARD(h, {
    if (state) ccz::free_state(h, static_cast<ccz::CpState*>(state));
  })
}

int ccz_cp_setup(ccz_handle h, void* state, const double* M_dev) {
  CCZ_GUARD(h, {
    ccz::CpState& S = *ccz::as_state<ccz::CpState>("cp", state);
    if (!M_dev) ccz::fail(CCZ_EINVAL, "cp: null tensor");
    S.restart(h);
    S.ready = false;
    ccz::cp_setup(h, S, M_dev);
    S.ready = true;
  })
}

int ccz_cp_set_init(ccz_handle h, void* state, const double* factors_host) {
  CCZ_GUARD(h, {
    ccz::CpState& S = *ccz::as_state<ccz::CpState>("cp", state);
    if (!S.ready) ccz::fail(CCZ_EINVAL, "cp: ccz_cp_setup has not been called");
    if (!factors_host) ccz::fail(CCZ_EINVAL, "cp: null initial factors");
    S.restart(h);
    ccz::h2d(h, S.B.A, factors_host, size_t(S.atot) * 8);
    ccz::cp_grams_and_start(h, S, false);
  })
}

int ccz_cp_iterations(ccz_handle h, void* state, int64_t n_iters, int64_t* iters_known, int* stopped_known) {
  CCZ_GUARD(h, {
    ccz::CpState& S = *ccz::as_state<ccz::CpState>("cp", state);
    if (!S.ready) ccz::fail(CCZ_EINVAL, "cp: ccz_cp_setup has not been called");
    ccz::run_chunk(h, "cp", "n_iters", S, n_iters, iters_known, stopped_known, &ccz::CpStatus::iters, [] { return 0; },
                   [&](int, int64_t) { ccz::enqueue_iteration(h, S); });
  })
}

int ccz_cp_status(ccz_handle h, void* state, int64_t* iters, int* stopped, int* reason, double* err, double* decrease) {
  CCZ_GUARD(h, {
    ccz::CpState& S = *ccz::as_state<ccz::CpState>("cp", state);
    if (!S.ready) ccz::fail(CCZ_EINVAL, "cp: ccz_cp_setup has not been called");
    const ccz::CpStatus st = ccz::read_status(h, S);
    if (iters) *iters = st.iters;
    if (stopped) *stopped = st.stopped;
    if (reason) *reason = st.reason;
    if (err) *err = st.err;
    if (decrease) *decrease = st.dec;
  })
}

int ccz_cp_get_result(ccz_handle h, void* state, double* factors_host, double* trace_host, int64_t* n_trace) {
  CCZ_GUARD(h, {
    ccz::CpState& S = *ccz::as_state<ccz::CpState>("cp", state);
    if (!S.ready) ccz::fail(CCZ_EINVAL, "cp: ccz_cp_setup has not been called");
    const ccz::CpStatus st = ccz::read_status(h, S);
    if (factors_host) ccz::d2h(h, factors_host, S.B.A, size_t(S.atot) * 8);
    if (trace_host && st.iters > 0) ccz::d2h(h, trace_host, S.B.trace, size_t(st.iters) * 8);
    if (n_trace) *n_trace = st.iters;
  })
}

}  // extern "C"
