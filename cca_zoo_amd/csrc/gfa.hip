// GFA (group factor analysis, Bayesian CCA with per-view ARD): whole coordinate-ascent iterations on the device.
//
// Reference: cca_zoo/probabilistic/_gfa.py:184-204 (initialisation), :217-286 (one iteration), the update equations of the
// R package CCAGFA.  The state is z (n x k), cov_z, zz = z'z + n cov_z, and per view w_m (p_m x k), cov_w[m],
// ww_m = w_m'w_m + p_m cov_w[m], alpha[m] (k), tau[m].  One iteration, for M views, in the reference's order of updates:
//   k_gfa_covw              one workgroup per view: cov_w[m] = (t t' / tau_m) o inv(t t' o zz + I / tau_m), t = alpha_m^-1/2
//   per view m:
//     k_gfa_xtz_*           column strips x row chunks: per-chunk partial sums of (X_m - mu_m)' z          (p_m x k)
//     k_gfa_wfold           the chunk partials summed in chunk order, w_m = (X_m' z) cov_w[m] tau_m, per-workgroup partial w_m'w_m
//   k_gfa_covz              one workgroup: ww_m, cov_z = inv(I + sum_m tau_m ww_m)
//   per view m:
//     k_gfa_xw_*            row blocks x column splits: partial sums of XW_m = (X_m - mu_m) w_m            (n x k)
//   k_gfa_z                 XW_m = its splits in split order, z = (sum_m tau_m XW_m) cov_z; per-workgroup partial z'z,
//                           sum z o XW_m per view, |z - z_prev|^2, |z_prev|^2
//   k_gfa_finish            one workgroup: zz, alpha, tau; the drop rule (mean z^2 > 1e-7 keeps a column; applied when some but
//                           not all columns are kept) compacts every k x k / k quantity; the stable counter, the stop
//   k_gfa_compact           after a prune only: the kept columns of z and w move to the front, in order
// After a prune the active k is smaller than the allocated one; the leading dimensions stay, every kernel reads the active k
// from the status word.  Every kernel reads that word first and returns at once when the fit has stopped; the host never
// waits inside a chunk.  All reductions run in a fixed order (partials, then folds in index order; no floating-point
// atomics): two fits of the same inputs give the same bits, whatever the chunk length.
//
// The two products run on v_mfma_f64_16x16x4f64 when the allocated k exceeds 4 (lane maps as in als.hip's k_als_gram: A operand
// m = lane & 15, k = lane >> 4; B operand k = lane >> 4, n = lane & 15; C/D col = lane & 15, row = (lane >> 4) + 4 reg), on
// plain FMAs below.  A lane loads 4 consecutive features (row_load.h), so operand index i of an MFMA stands for feature
// 4 i + q of the lane group, q = 0..3 one MFMA each.
//
// Precision: x - mu is rounded in the views' precision (the reference centres in the input dtype, then promotes), then
// widened; every product and sum is fp64.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <vector>

#include "hip_common.h"
#include "abi_guard.h"
#include "fit_driver.h"
#include "reduce.h"
#include "row_load.h"

namespace ccz {

namespace {

constexpr int GFA_MAXV = 8;            // views per fit
constexpr int GFA_MAXK = 32;           // latent dimensions per fit; also the leading dimension of every k x k matrix
constexpr int GFA_KK = GFA_MAXK * GFA_MAXK;
constexpr int GFA_LD = GFA_MAXK + 1;   // LDS row stride of a k x k matrix (doubles)
constexpr int GFA_PT = 1024;           // threads of the one-workgroup kernels: one per k x k entry
constexpr int GFA_G = 256;             // most workgroups of a kernel that leaves k x k partials
constexpr int GFA_FB = 64;             // k_gfa_wfold: features per pass of a workgroup
constexpr int GFA_ZR = 8;              // k_gfa_z: rows per pass of a workgroup
constexpr int GFA_ZP = GFA_KK + GFA_MAXV + 2;   // k_gfa_z partials per workgroup: z'z, sum z o XW_m, |z - z_prev|^2, |z_prev|^2
constexpr int GFA_PLAIN_K = 4;         // allocated k up to which the products run on plain FMAs
constexpr int GFA_XROWS = 64;          // k_gfa_xw_mfma: rows per workgroup (4 MFMA row tiles)
constexpr int GFA_SROWS = 4;           // k_gfa_xw_plain: rows per workgroup
constexpr int GFA_CSMAX = 16;          // most column splits of k_gfa_xw_*
constexpr int GFA_PATIENCE = 1000;     // cca_zoo/probabilistic/_gfa.py:19
constexpr int64_t GFA_SCRATCH_BYTES = int64_t(512) << 20;   // budget of the X'z chunk partials (nchunk x p_max x k doubles)

constexpr double GFA_PRIOR = 1e-14;    // _ARD_ALPHA_0 = _ARD_BETA_0 = _TAU_ALPHA_0 = _TAU_BETA_0
constexpr double GFA_INIT_TAU = 1e3;
constexpr double GFA_DROP_TOL = 1e-7;

typedef double v4f64 __attribute__((ext_vector_type(4)));

struct GfaStatus {
  double rel_change;               // of the last iteration that formed it
  long long iters;                 // iterations done
  int k;                           // active latent dimensions
  int stable;                      // consecutive iterations with rel_change < tol and no prune
  int stopped;
  int pruned;                      // the last finish pruned (read by k_gfa_compact)
  int nprune;
  int keep[GFA_MAXK];              // the last prune: old index of new column j
  long long prune_iter[GFA_MAXK];  // iteration (1-based) of every prune
  int prune_k[GFA_MAXK];           // active k after it
};

struct GfaViews {
  const void* X[GFA_MAXV];
  const void* mu[GFA_MAXV];
  int64_t ld[GFA_MAXV];
  int64_t p[GFA_MAXV];
  int64_t off[GFA_MAXV];           // offset of view m in the concatenated rows of w
  int64_t xwoff[GFA_MAXV];         // offset (doubles) of view m's split partials in xwpart
  int cs[GFA_MAXV];                // column splits of k_gfa_xw_*
  int gw[GFA_MAXV];                // workgroups of k_gfa_wfold
};

// the device buffers of one fit; k x k matrices have leading dimension GFA_MAXK, z / w / XW the allocated k (K)
struct GfaBuf {
  double* z;        // n x K
  double* w;        // ptot x K
  double* xw;       // M x n x K
  double* xwpart;   // per view cs x n x K: column-split partial sums of XW_m
  double* xpart;    // nchunk x pmax x K: row-chunk partial sums of X' z
  double* covz;     // KK
  double* zz;       // KK
  double* covw;     // M x KK
  double* ww;       // M x KK
  double* alpha;    // M x MAXK
  double* bard;     // M x MAXK
  double* tau;      // M
  double* btau;     // M
  double* yconst;   // M: sum fl(x - mu)^2
  double* datavar;  // M: sum over the columns of the ddof = 1 variance of fl(x - mu)
  double* wwpart;   // M x GFA_G x KK
  double* zpart;    // GFA_G x GFA_ZP
  double* cmean;    // pmax: float64 column means of fl(x - mu) (setup)
  int n, M, K, nchunk, rc, gz, sc, src;
  int64_t ptot, pmax;
  double tol;
  int max_iter, drop_k;
};

// X = A^-1 for a symmetric positive definite k x k A in LDS (row stride GFA_LD), as the reference forms it: the lower Cholesky
// factor L (left in A's lower triangle), Y = L^-1, X = L^-T Y (cca_zoo/probabilistic/_gfa.py:222-223).  Whole workgroup;
// thread t < k owns row t of L and column t of Y and X.  A non-positive pivot gives NaNs, which reach the weights.
__device__ void gfa_spd_inverse(double* A, double* Y, double* X, int k) {
  const int t = threadIdx.x;
  for (int j = 0; j < k; ++j) {
    __syncthreads();
    if (t == 0) {
      double s = A[j * GFA_LD + j];
      for (int l = 0; l < j; ++l) s -= A[j * GFA_LD + l] * A[j * GFA_LD + l];
      A[j * GFA_LD + j] = sqrt(s);
    }
    __syncthreads();
    if (t > j && t < k) {
      double s = A[t * GFA_LD + j];
      for (int l = 0; l < j; ++l) s -= A[t * GFA_LD + l] * A[j * GFA_LD + l];
      A[t * GFA_LD + j] = s / A[j * GFA_LD + j];
    }
  }
  __syncthreads();
  if (t < k) {
    for (int i = 0; i < k; ++i) {
      double s = i == t ? 1.0 : 0.0;
      for (int l = 0; l < i; ++l) s -= A[i * GFA_LD + l] * Y[l * GFA_LD + t];
      Y[i * GFA_LD + t] = s / A[i * GFA_LD + i];
    }
    for (int i = k - 1; i >= 0; --i) {
      double s = Y[i * GFA_LD + t];
      for (int l = i + 1; l < k; ++l) s -= A[l * GFA_LD + i] * X[l * GFA_LD + t];
      X[i * GFA_LD + t] = s / A[i * GFA_LD + i];
    }
  }
  __syncthreads();
}

// ---- cov_w (cca_zoo/probabilistic/_gfa.py:220-224) --------------------------------------------------------------------
__global__ void __launch_bounds__(256) k_gfa_covw(GfaBuf B, const GfaStatus* st) {
  if (fit_stopped(st)) return;
  __shared__ double A[GFA_MAXK * GFA_LD], Y[GFA_MAXK * GFA_LD], X[GFA_MAXK * GFA_LD];
  __shared__ double tmp[GFA_MAXK];
  const int m = blockIdx.x, k = st->k, t = threadIdx.x;
  const double tau = B.tau[m];
  if (t < k) tmp[t] = 1.0 / sqrt(B.alpha[m * GFA_MAXK + t]);
  __syncthreads();
  for (int e = t; e < GFA_KK; e += 256) {
    const int a = e >> 5, b = e & 31;
    if (a < k && b < k) A[a * GFA_LD + b] = (tmp[a] * tmp[b]) * B.zz[e] + (a == b ? 1.0 / tau : 0.0);
  }
  gfa_spd_inverse(A, Y, X, k);
  for (int e = t; e < GFA_KK; e += 256) {
    const int a = e >> 5, b = e & 31;
    if (a < k && b < k) B.covw[m * GFA_KK + e] = ((1.0 / tau) * (tmp[a] * tmp[b])) * X[a * GFA_LD + b];
  }
}

// ---- X' z: per-chunk partial sums ---------------------------------------------------------------------------------------
// plain: grid (ceil(p / 1024), nchunk), 256 threads; thread t owns columns 1024 bx + 4 t .. + 3 over rows [rc by, rc (by + 1))
template <typename T>
__global__ void __launch_bounds__(256) k_gfa_xtz_plain(const T* __restrict__ X, const T* __restrict__ mu, int64_t ld, int64_t p, int n,
                                                      int rc, int K, const double* __restrict__ z, double* __restrict__ xpart,
                                                      const GfaStatus* st) {
  if (fit_stopped(st)) return;
  const int k = st->k;
  const int64_t f0 = int64_t(blockIdx.x) * 1024 + 4 * threadIdx.x;
  if (f0 >= p) return;
  const int r0 = blockIdx.y * rc, r1 = min(n, r0 + rc);
  const bool vec = vec_ok(X, ld, mu);
  T m[4] = {T(0), T(0), T(0), T(0)};
  if (mu) load4<T>(mu, f0, p, vec, m);
  double acc[4][GFA_PLAIN_K];
#pragma unroll
  for (int q = 0; q < 4; ++q)
#pragma unroll
    for (int a = 0; a < GFA_PLAIN_K; ++a) acc[q][a] = 0.0;
#pragma unroll 2
  for (int r = r0; r < r1; ++r) {
    T x[4];
    load4<T>(X + int64_t(r) * ld, f0, p, vec, x);
    double zr[GFA_PLAIN_K];
#pragma unroll
    for (int a = 0; a < GFA_PLAIN_K; ++a) zr[a] = a < k ? z[int64_t(r) * K + a] : 0.0;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const double xc = double(T(x[q] - m[q]));
#pragma unroll
      for (int a = 0; a < GFA_PLAIN_K; ++a) acc[q][a] += xc * zr[a];
    }
  }
  double* out = xpart + int64_t(blockIdx.y) * p * K;
#pragma unroll
  for (int q = 0; q < 4; ++q)
#pragma unroll
    for (int a = 0; a < GFA_PLAIN_K; ++a)
      if (f0 + q < p && a < k) out[(f0 + q) * K + a] = acc[q][a];
}

// MFMA: grid (ceil(p / 256), nchunk), 256 threads; wave w owns features 256 bx + 64 w .. + 63, lane group li = lane & 15 the
// four features 4 li + q; rows go through the contraction four at a time (lane >> 4).  KT = tiles of 16 latent columns.
template <typename T, int KT>
__global__ void __launch_bounds__(256) k_gfa_xtz_mfma(const T* __restrict__ X, const T* __restrict__ mu, int64_t ld, int64_t p, int n,
                                                     int rc, int K, const double* __restrict__ z, double* __restrict__ xpart,
                                                     const GfaStatus* st) {
  if (fit_stopped(st)) return;
  const int k = st->k;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int li = lane & 15, lg = lane >> 4;
  const int64_t fw = int64_t(blockIdx.x) * 256 + 64 * wave;
  if (fw >= p) return;
  const int64_t f0 = fw + 4 * li;
  const int r0 = blockIdx.y * rc, r1 = min(n, r0 + rc);
  const bool vec = vec_ok(X, ld, mu);
  T m[4] = {T(0), T(0), T(0), T(0)};
  if (mu && f0 < p) load4<T>(mu, f0, p, vec, m);
  v4f64 acc[4][KT];
#pragma unroll
  for (int q = 0; q < 4; ++q)
#pragma unroll
    for (int kt = 0; kt < KT; ++kt) acc[q][kt] = v4f64{0.0, 0.0, 0.0, 0.0};
  for (int r = r0; r < r1; r += 4) {
    const int rr = r + lg;
    const bool ok = rr < r1;
    T x[4] = {T(0), T(0), T(0), T(0)};
    if (ok && f0 < p) load4<T>(X + int64_t(rr) * ld, f0, p, vec, x);
    double xc[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) xc[q] = (ok && f0 + q < p) ? double(T(x[q] - m[q])) : 0.0;
#pragma unroll
    for (int kt = 0; kt < KT; ++kt) {
      if (16 * kt >= k) break;
      const int col = 16 * kt + li;
      const double zv = (ok && col < k) ? z[int64_t(rr) * K + col] : 0.0;
#pragma unroll
      for (int q = 0; q < 4; ++q) acc[q][kt] = __builtin_amdgcn_mfma_f64_16x16x4f64(xc[q], zv, acc[q][kt], 0, 0, 0);
    }
  }
  double* out = xpart + int64_t(blockIdx.y) * p * K;
#pragma unroll
  for (int kt = 0; kt < KT; ++kt) {
    const int col = 16 * kt + li;
    if (col >= k) continue;
#pragma unroll
    for (int q = 0; q < 4; ++q)
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        const int64_t f = fw + 4 * (lg + 4 * g) + q;
        if (f < p) out[f * K + col] = acc[q][kt][g];
      }
  }
}

// ---- w_m and the partial sums of w_m' w_m (cca_zoo/probabilistic/_gfa.py:225-226) ----------------------------------------
// grid gw <= GFA_G workgroups of 256 threads; workgroup b takes feature blocks b, b + gw, ... of 64 features
__global__ void __launch_bounds__(256) k_gfa_wfold(GfaBuf B, int m, int64_t p, int64_t off, const GfaStatus* st) {
  if (fit_stopped(st)) return;
  __shared__ double xz[GFA_FB * GFA_LD], wt[GFA_FB * GFA_LD], cw[GFA_MAXK * GFA_LD];
  const int k = st->k, K = B.K, t = threadIdx.x;
  const double tau = B.tau[m];
  for (int e = t; e < GFA_KK; e += 256) {
    const int a = e >> 5, b = e & 31;
    cw[a * GFA_LD + b] = (a < k && b < k) ? B.covw[m * GFA_KK + e] : 0.0;
  }
  double acc[4] = {0.0, 0.0, 0.0, 0.0};
  const int64_t nblk = (p + GFA_FB - 1) / GFA_FB;
  for (int64_t blk = blockIdx.x; blk < nblk; blk += gridDim.x) {
    const int64_t f0 = blk * GFA_FB;
    __syncthreads();
    for (int e = t; e < GFA_FB * K; e += 256) {
      const int fl = e / K, a = e % K;
      const int64_t f = f0 + fl;
      double v = 0.0;
      if (f < p && a < k)
        for (int c = 0; c < B.nchunk; ++c) v += B.xpart[(int64_t(c) * p + f) * K + a];
      xz[fl * GFA_LD + a] = v;
    }
    __syncthreads();
    for (int e = t; e < GFA_FB * K; e += 256) {
      const int fl = e / K, b = e % K;
      const int64_t f = f0 + fl;
      double s = 0.0;
      if (f < p && b < k) {
        for (int a = 0; a < k; ++a) s += xz[fl * GFA_LD + a] * cw[a * GFA_LD + b];
        s *= tau;
        B.w[(off + f) * K + b] = s;
      }
      wt[fl * GFA_LD + b] = s;
    }
    __syncthreads();
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int e = t + 256 * j, a = e >> 5, b = e & 31;
      if (a < k && b < k)
        for (int fl = 0; fl < GFA_FB; ++fl) acc[j] += wt[fl * GFA_LD + a] * wt[fl * GFA_LD + b];
    }
  }
  double* out = B.wwpart + (int64_t(m) * GFA_G + blockIdx.x) * GFA_KK;
#pragma unroll
  for (int j = 0; j < 4; ++j) out[t + 256 * j] = acc[j];
}

// ---- ww_m and cov_z (cca_zoo/probabilistic/_gfa.py:226-233) ---------------------------------------------------------------
__global__ void __launch_bounds__(GFA_PT) k_gfa_covz(GfaBuf B, GfaViews vw, const GfaStatus* st) {
  if (fit_stopped(st)) return;
  __shared__ double A[GFA_MAXK * GFA_LD], Y[GFA_MAXK * GFA_LD], X[GFA_MAXK * GFA_LD];
  const int k = st->k, e = threadIdx.x, a = e >> 5, b = e & 31;
  const bool in = a < k && b < k;
  double prec = a == b ? 1.0 : 0.0;
  for (int m = 0; m < B.M; ++m) {
    double s = 0.0;
    if (in) {
      const double* part = B.wwpart + int64_t(m) * GFA_G * GFA_KK;
      for (int g = 0; g < vw.gw[m]; ++g) s += part[int64_t(g) * GFA_KK + e];
      s += double(vw.p[m]) * B.covw[m * GFA_KK + e];
      B.ww[m * GFA_KK + e] = s;
    }
    prec = prec + B.tau[m] * s;
  }
  if (in) A[a * GFA_LD + b] = prec;
  gfa_spd_inverse(A, Y, X, k);
  if (in) B.covz[e] = X[a * GFA_LD + b];
}

// ---- X w: column-split partial sums -------------------------------------------------------------------------------------
// plain: grid (ceil(n / 4), cs), 256 threads: 4 rows x one column range per workgroup, 4 consecutive columns per thread and step
template <typename T>
__global__ void __launch_bounds__(256) k_gfa_xw_plain(const T* __restrict__ X, const T* __restrict__ mu, int64_t ld, int64_t p, int n,
                                                     int K, const double* __restrict__ w, double* __restrict__ part,
                                                     const GfaStatus* st) {
  if (fit_stopped(st)) return;
  __shared__ double sh[4];
  const int k = st->k;
  const int r0 = blockIdx.x * GFA_SROWS;
  int64_t c0, c1;
  split_range(p, gridDim.y, int(blockIdx.y), &c0, &c1);
  const bool vec = vec_ok(X, ld, mu);
  double acc[GFA_SROWS][GFA_PLAIN_K];
#pragma unroll
  for (int t = 0; t < GFA_SROWS; ++t)
#pragma unroll
    for (int a = 0; a < GFA_PLAIN_K; ++a) acc[t][a] = 0.0;
  const T* rowp[GFA_SROWS];
  bool live[GFA_SROWS];
#pragma unroll
  for (int t = 0; t < GFA_SROWS; ++t) {
    live[t] = r0 + t < n;
    rowp[t] = X + int64_t(live[t] ? r0 + t : 0) * ld;
  }
  for (int64_t f0 = c0 + 4 * threadIdx.x; f0 < c1; f0 += 1024) {
    double wv[4][GFA_PLAIN_K];
#pragma unroll
    for (int q = 0; q < 4; ++q)
#pragma unroll
      for (int a = 0; a < GFA_PLAIN_K; ++a) wv[q][a] = (f0 + q < c1 && a < k) ? w[(f0 + q) * K + a] : 0.0;
    T m[4] = {T(0), T(0), T(0), T(0)};
    if (mu) load4<T>(mu, f0, c1, vec, m);
#pragma unroll
    for (int t = 0; t < GFA_SROWS; ++t) {
      if (!live[t]) continue;
      T x[4];
      load4<T>(rowp[t], f0, c1, vec, x);
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const double xc = double(T(x[q] - m[q]));
#pragma unroll
        for (int a = 0; a < GFA_PLAIN_K; ++a) acc[t][a] += xc * wv[q][a];
      }
    }
  }
#pragma unroll
  for (int t = 0; t < GFA_SROWS; ++t)
#pragma unroll
    for (int a = 0; a < GFA_PLAIN_K; ++a) {
      const double s = block_sum<4>(acc[t][a], sh);
      if (threadIdx.x == 0 && live[t] && a < k) part[(int64_t(blockIdx.y) * n + r0 + t) * K + a] = s;
    }
}

// MFMA: grid (ceil(n / 64), cs), 256 threads: 64 rows (4 row tiles) x one column range per workgroup; wave w takes the feature
// blocks c0 + 16 w + 64 j, lane group lg = lane >> 4 the four features 4 lg + q of a block; the four waves are summed in wave order
template <typename T, int KT>
__global__ void __launch_bounds__(256) k_gfa_xw_mfma(const T* __restrict__ X, const T* __restrict__ mu, int64_t ld, int64_t p, int n,
                                                    int K, const double* __restrict__ w, double* __restrict__ part,
                                                    const GfaStatus* st) {
  if (fit_stopped(st)) return;
  __shared__ double red[4][GFA_XROWS][16];
  const int k = st->k;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int li = lane & 15, lg = lane >> 4;
  const int64_t R0 = int64_t(blockIdx.x) * GFA_XROWS;
  int64_t c0, c1;
  split_range(p, gridDim.y, int(blockIdx.y), &c0, &c1);
  const bool vec = vec_ok(X, ld, mu);
  v4f64 acc[4][KT];
#pragma unroll
  for (int t = 0; t < 4; ++t)
#pragma unroll
    for (int kt = 0; kt < KT; ++kt) acc[t][kt] = v4f64{0.0, 0.0, 0.0, 0.0};
  for (int64_t fb = c0 + 16 * wave; fb < c1; fb += 64) {
    const int64_t f0 = fb + 4 * lg;
    T m[4] = {T(0), T(0), T(0), T(0)};
    if (mu && f0 < c1) load4<T>(mu, f0, c1, vec, m);
    double wv[4][KT];
#pragma unroll
    for (int q = 0; q < 4; ++q)
#pragma unroll
      for (int kt = 0; kt < KT; ++kt) {
        const int col = 16 * kt + li;
        wv[q][kt] = (f0 + q < c1 && col < k) ? w[(f0 + q) * K + col] : 0.0;
      }
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      const int64_t row = R0 + 16 * t + li;
      const bool live = row < n && f0 < c1;
      T x[4] = {T(0), T(0), T(0), T(0)};
      if (live) load4<T>(X + row * ld, f0, c1, vec, x);
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const double xc = (live && f0 + q < c1) ? double(T(x[q] - m[q])) : 0.0;
#pragma unroll
        for (int kt = 0; kt < KT; ++kt) {
          if (16 * kt >= k) break;
          acc[t][kt] = __builtin_amdgcn_mfma_f64_16x16x4f64(xc, wv[q][kt], acc[t][kt], 0, 0, 0);
        }
      }
    }
  }
#pragma unroll
  for (int kt = 0; kt < KT; ++kt) {
    if (16 * kt >= k) break;
    __syncthreads();
#pragma unroll
    for (int t = 0; t < 4; ++t)
#pragma unroll
      for (int g = 0; g < 4; ++g) red[wave][16 * t + lg + 4 * g][li] = acc[t][kt][g];
    __syncthreads();
    for (int e = threadIdx.x; e < GFA_XROWS * 16; e += 256) {
      const int rr = e >> 4, cc = e & 15;
      const int64_t row = R0 + rr;
      const int col = 16 * kt + cc;
      if (row < n && col < k)
        part[(int64_t(blockIdx.y) * n + row) * K + col] = ((red[0][rr][cc] + red[1][rr][cc]) + red[2][rr][cc]) + red[3][rr][cc];
    }
  }
}

// ---- z and its partial sums (cca_zoo/probabilistic/_gfa.py:234-238, :252, :261, :279) --------------------------------------
// grid gz <= GFA_G workgroups of 256 threads; workgroup b takes row blocks b, b + gz, ... of 8 rows; thread (row t >> 5, column t & 31)
__global__ void __launch_bounds__(256) k_gfa_z(GfaBuf B, GfaViews vw, const GfaStatus* st) {
  if (fit_stopped(st)) return;
  __shared__ double cz[GFA_MAXK * GFA_LD], rhs[GFA_ZR * GFA_LD], zt[GFA_ZR * GFA_LD];
  __shared__ double sh[4];
  const int k = st->k, K = B.K, n = B.n, M = B.M, t = threadIdx.x;
  const int rl = t >> 5, col = t & 31;
  for (int e = t; e < GFA_KK; e += 256) {
    const int a = e >> 5, b = e & 31;
    cz[a * GFA_LD + b] = (a < k && b < k) ? B.covz[e] : 0.0;
  }
  double tau[GFA_MAXV], zx[GFA_MAXV];
#pragma unroll
  for (int m = 0; m < GFA_MAXV; ++m) {
    tau[m] = m < M ? B.tau[m] : 0.0;
    zx[m] = 0.0;
  }
  double acc[4] = {0.0, 0.0, 0.0, 0.0};
  double dd = 0.0, pp = 0.0;
  const int64_t nblk = (int64_t(n) + GFA_ZR - 1) / GFA_ZR;
  for (int64_t blk = blockIdx.x; blk < nblk; blk += gridDim.x) {
    const int64_t r = blk * GFA_ZR + rl;
    const bool live = r < n && col < k;
    double xwv[GFA_MAXV];
    double s = 0.0;
#pragma unroll
    for (int m = 0; m < GFA_MAXV; ++m) {
      double v = 0.0;
      if (m < M && live) {
        const double* part = B.xwpart + vw.xwoff[m];
        for (int c = 0; c < vw.cs[m]; ++c) v += part[(int64_t(c) * n + r) * K + col];
        B.xw[(int64_t(m) * n + r) * K + col] = v;
        s = s + v * tau[m];
      }
      xwv[m] = v;
    }
    __syncthreads();
    rhs[rl * GFA_LD + col] = live ? s : 0.0;
    __syncthreads();
    double zn = 0.0;
    if (live) {
      for (int a = 0; a < k; ++a) zn += rhs[rl * GFA_LD + a] * cz[a * GFA_LD + col];
      const double zp = B.z[r * K + col], d = zn - zp;
      dd += d * d;
      pp += zp * zp;
      B.z[r * K + col] = zn;
#pragma unroll
      for (int m = 0; m < GFA_MAXV; ++m) zx[m] += zn * xwv[m];
    }
    zt[rl * GFA_LD + col] = zn;
    __syncthreads();
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int e = t + 256 * j, a = e >> 5, b = e & 31;
      if (a < k && b < k)
        for (int q = 0; q < GFA_ZR; ++q) acc[j] += zt[q * GFA_LD + a] * zt[q * GFA_LD + b];
    }
  }
  double* out = B.zpart + int64_t(blockIdx.x) * GFA_ZP;
#pragma unroll
  for (int j = 0; j < 4; ++j) out[t + 256 * j] = acc[j];
#pragma unroll
  for (int m = 0; m < GFA_MAXV; ++m) {
    const double s = block_sum<4>(zx[m], sh);
    if (t == 0) out[GFA_KK + m] = s;
  }
  dd = block_sum<4>(dd, sh);
  pp = block_sum<4>(pp, sh);
  if (t == 0) {
    out[GFA_KK + GFA_MAXV] = dd;
    out[GFA_KK + GFA_MAXV + 1] = pp;
  }
}

// out[e] = src[keep[a] x keep[b]] for a k x k matrix, in place, by the whole workgroup (thread e = 32 a + b)
__device__ __forceinline__ void gfa_compact_kk(double* Mx, const int* keep, int nk) {
  const int e = threadIdx.x, a = e >> 5, b = e & 31;
  const bool in = a < nk && b < nk;
  const double v = in ? Mx[keep[a] * GFA_MAXK + keep[b]] : 0.0;
  __syncthreads();
  if (in) Mx[e] = v;
  __syncthreads();
}

// once per iteration: zz, alpha, tau, the drop rule, the stable counter and the stop (cca_zoo/probabilistic/_gfa.py:238-286)
__global__ void __launch_bounds__(GFA_PT) k_gfa_finish(GfaBuf B, GfaViews vw, GfaStatus* st) {
  if (fit_stopped(st)) {
    if (threadIdx.x == 0) st->pruned = 0;
    return;
  }
  __shared__ double sh[GFA_PT / 64];
  __shared__ double z2[GFA_MAXK];
  __shared__ int keep[GFA_MAXK];
  __shared__ int nkeep, prune;
  const int k = st->k, M = B.M, n = B.n, e = threadIdx.x, a = e >> 5, b = e & 31;
  const bool in = a < k && b < k;
  double s = 0.0;
  if (in)
    for (int g = 0; g < B.gz; ++g) s += B.zpart[int64_t(g) * GFA_ZP + e];
  const double zzv = in ? s + double(n) * B.covz[e] : 0.0;
  if (in) B.zz[e] = zzv;
  if (in && a == b) z2[a] = s / double(n);
  const double dd = block_sum<GFA_PT / 64>(e < B.gz ? B.zpart[int64_t(e) * GFA_ZP + GFA_KK + GFA_MAXV] : 0.0, sh);
  const double pp = block_sum<GFA_PT / 64>(e < B.gz ? B.zpart[int64_t(e) * GFA_ZP + GFA_KK + GFA_MAXV + 1] : 0.0, sh);
  if (e < M * GFA_MAXK) {
    const int m = e >> 5, c = e & 31;
    if (c < k) {
      const double bard = GFA_PRIOR + B.ww[m * GFA_KK + c * GFA_MAXK + c] / 2.0;
      B.bard[m * GFA_MAXK + c] = bard;
      B.alpha[m * GFA_MAXK + c] = (GFA_PRIOR + double(vw.p[m]) / 2.0) / bard;
    }
  }
  for (int m = 0; m < M; ++m) {
    const double zx = block_sum<GFA_PT / 64>(e < B.gz ? B.zpart[int64_t(e) * GFA_ZP + GFA_KK + m] : 0.0, sh);
    const double wz = block_sum<GFA_PT / 64>(in ? B.ww[m * GFA_KK + e] * zzv : 0.0, sh);
    if (e == 0) {
      const double btau = GFA_PRIOR + (B.yconst[m] + wz - 2.0 * zx) / 2.0;
      B.btau[m] = btau;
      B.tau[m] = (GFA_PRIOR + double(n) * double(vw.p[m]) / 2.0) / btau;
    }
  }
  if (e == 0) {
    int nk = 0;
    if (B.drop_k)
      for (int c = 0; c < k; ++c)
        if (z2[c] > GFA_DROP_TOL) keep[nk++] = c;
    nkeep = nk;
    prune = (B.drop_k && nk > 0 && nk != k) ? 1 : 0;
  }
  __syncthreads();
  if (prune) {
    const int nk = nkeep;
    gfa_compact_kk(B.covz, keep, nk);
    gfa_compact_kk(B.zz, keep, nk);
    for (int m = 0; m < M; ++m) {
      gfa_compact_kk(B.covw + m * GFA_KK, keep, nk);
      gfa_compact_kk(B.ww + m * GFA_KK, keep, nk);
    }
    const int m = e >> 5, c = e & 31;
    const bool inv = e < M * GFA_MAXK && c < nk;
    const double al = inv ? B.alpha[m * GFA_MAXK + keep[c]] : 0.0, ba = inv ? B.bard[m * GFA_MAXK + keep[c]] : 0.0;
    __syncthreads();
    if (inv) {
      B.alpha[m * GFA_MAXK + c] = al;
      B.bard[m * GFA_MAXK + c] = ba;
    }
  }
  if (e == 0) {
    const long long it = st->iters + 1;
    int stable = st->stable;
    st->iters = it;
    if (prune) {
      for (int c = 0; c < nkeep; ++c) st->keep[c] = keep[c];
      st->k = nkeep;
      st->prune_iter[st->nprune] = it;
      st->prune_k[st->nprune] = nkeep;
      st->nprune += 1;
      st->pruned = 1;
      stable = 0;
    } else {
      st->pruned = 0;
      if (it > 1) {     // the first iteration has no previous z
        const double rel = sqrt(dd) / fmax(sqrt(pp), 1e-300);
        st->rel_change = rel;
        stable = rel < B.tol ? stable + 1 : 0;
      }
    }
    st->stable = stable;
    if (stable >= GFA_PATIENCE || it >= B.max_iter) st->stopped = 1;
  }
}

// after a prune: the kept columns of every row of z and w move to the front (keep[j] >= j and ascending: in place)
__global__ void __launch_bounds__(256) k_gfa_compact(GfaBuf B, const GfaStatus* st) {
  if (!st->pruned) return;
  const int nk = st->k, K = B.K;
  const int64_t rows = int64_t(B.n) + B.ptot;
  for (int64_t r = int64_t(blockIdx.x) * 256 + threadIdx.x; r < rows; r += int64_t(gridDim.x) * 256) {
    double* row = r < B.n ? B.z + r * K : B.w + (r - B.n) * K;
    for (int j = 0; j < nk; ++j) row[j] = row[st->keep[j]];
  }
}

// ---- setup: y_const, datavar, the initial state (cca_zoo/probabilistic/_gfa.py:184-204) -----------------------------------
// grid (ceil(p / 256), sc), one thread per column over a row chunk.  pass 0: partial sums of xc = fl(x - mu) and of xc^2;
// pass 1: partial sums of (xc - cmean)^2, cmean the float64 mean of the column of xc (np.var re-centres)
template <typename T>
__global__ void __launch_bounds__(256) k_gfa_stat(const T* __restrict__ X, const T* __restrict__ mu, int64_t ld, int64_t p, int n, int rc,
                                                 int pass, const double* __restrict__ cmean, double* __restrict__ part) {
  const int64_t f = int64_t(blockIdx.x) * 256 + threadIdx.x;
  if (f >= p) return;
  const int r0 = blockIdx.y * rc, r1 = min(n, r0 + rc);
  const T m = mu ? mu[f] : T(0);
  const double cm = pass ? cmean[f] : 0.0;
  double s = 0.0, s2 = 0.0;
  for (int r = r0; r < r1; ++r) {
    const double xc = double(T(X[int64_t(r) * ld + f] - m)) - cm;
    s += xc;
    s2 += xc * xc;
  }
  part[(int64_t(blockIdx.y) * 2 + 0) * p + f] = s;
  part[(int64_t(blockIdx.y) * 2 + 1) * p + f] = s2;
}

// one workgroup: the chunk partials in chunk order per column, then the columns by strided per-thread sums and a block sum.
// pass 0: cmean[f], out[0] = sum of squares (y_const); pass 1: out[1] = sum of the ddof = 1 variances (datavar)
__global__ void __launch_bounds__(GFA_PT) k_gfa_stat_fold(const double* __restrict__ part, int sc, int64_t p, int n, int pass,
                                                         double* __restrict__ cmean, double* __restrict__ out0, double* __restrict__ out1) {
  __shared__ double sh[GFA_PT / 64];
  double tot = 0.0;
  for (int64_t f = threadIdx.x; f < p; f += GFA_PT) {
    double s = 0.0, s2 = 0.0;
    for (int c = 0; c < sc; ++c) {
      s += part[(int64_t(c) * 2 + 0) * p + f];
      s2 += part[(int64_t(c) * 2 + 1) * p + f];
    }
    if (!pass) cmean[f] = s / double(n);
    tot += pass ? s2 / double(n - 1) : s2;
  }
  tot = block_sum<GFA_PT / 64>(tot, sh);
  if (threadIdx.x == 0) *(pass ? out1 : out0) = tot;
}

// partial sums of z0' z0 in the layout of k_gfa_z
__global__ void __launch_bounds__(256) k_gfa_zz0(GfaBuf B) {
  const int K = B.K, t = threadIdx.x;
  double acc[4] = {0.0, 0.0, 0.0, 0.0};
  for (int64_t r = blockIdx.x; r < B.n; r += gridDim.x) {
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int e = t + 256 * j, a = e >> 5, b = e & 31;
      if (a < K && b < K) acc[j] += B.z[r * K + a] * B.z[r * K + b];
    }
  }
  double* out = B.zpart + int64_t(blockIdx.x) * GFA_ZP;
#pragma unroll
  for (int j = 0; j < 4; ++j) out[t + 256 * j] = acc[j];
}

// one workgroup: tau = 1e3, alpha = k p / max(datavar - 1 / tau, 1e-8), cov_z = cov_w = I, w = 0 so ww = p I, zz = z0'z0 + n I,
// b_ard = b_tau = 1e-14; the status word
__global__ void __launch_bounds__(GFA_PT) k_gfa_init(GfaBuf B, GfaViews vw, GfaStatus* st) {
  const int K = B.K, e = threadIdx.x, a = e >> 5, b = e & 31;
  const bool in = a < K && b < K;
  const double eye = a == b ? 1.0 : 0.0;
  double s = 0.0;
  if (in)
    for (int g = 0; g < B.gz; ++g) s += B.zpart[int64_t(g) * GFA_ZP + e];
  B.zz[e] = in ? s + double(B.n) * eye : 0.0;
  B.covz[e] = in ? eye : 0.0;
  for (int m = 0; m < B.M; ++m) {
    B.covw[m * GFA_KK + e] = in ? eye : 0.0;
    B.ww[m * GFA_KK + e] = in ? 0.0 + double(vw.p[m]) * eye : 0.0;
  }
  if (e < B.M * GFA_MAXK) {
    const int m = e >> 5, c = e & 31;
    B.alpha[e] = c < K ? double(K) * double(vw.p[m]) / fmax(B.datavar[m] - 1.0 / GFA_INIT_TAU, 1e-8) : 0.0;
    B.bard[e] = c < K ? GFA_PRIOR : 0.0;
  }
  if (e < B.M) {
    B.tau[e] = GFA_INIT_TAU;
    B.btau[e] = GFA_PRIOR;
  }
  if (e == 0) {
    st->rel_change = 0.0;
    st->iters = 0;
    st->k = K;
    st->stable = 0;
    st->stopped = 0;
    st->pruned = 0;
    st->nprune = 0;
  }
}

// ---- host driver ----------------------------------------------------------------------------------------------------
struct GfaState : FitState<GfaStatus> {
  int64_t n, K;
  GfaBuf B;
  GfaViews shape;                  // cs, gw, off, xwoff per view (the pointers are filled per call)
  bool has_init = false, ready = false;
};

GfaViews make_views(const GfaState& S, const ccz_view* views, const void* const* means) {
  GfaViews vw = S.shape;
  fill_views("gfa", vw, views, means, S.p);
  return vw;
}

template <typename T>
void launch_xtz(ccz_ctx* c, const GfaState& S, const GfaViews& vw, int i) {
  const GfaBuf& B = S.B;
  const T* X = static_cast<const T*>(vw.X[i]);
  const T* mu = static_cast<const T*>(vw.mu[i]);
  if (S.K <= GFA_PLAIN_K) {
    const dim3 grid(unsigned((vw.p[i] + 1023) / 1024), unsigned(B.nchunk));
    hipLaunchKernelGGL((k_gfa_xtz_plain<T>), grid, dim3(256), 0, stream(c), X, mu, vw.ld[i], vw.p[i], B.n, B.rc, B.K, B.z, B.xpart, S.drv.dev);
  } else {
    const dim3 grid(unsigned((vw.p[i] + 255) / 256), unsigned(B.nchunk));
    if (S.K <= 16)
      hipLaunchKernelGGL((k_gfa_xtz_mfma<T, 1>), grid, dim3(256), 0, stream(c), X, mu, vw.ld[i], vw.p[i], B.n, B.rc, B.K, B.z, B.xpart, S.drv.dev);
    else
      hipLaunchKernelGGL((k_gfa_xtz_mfma<T, 2>), grid, dim3(256), 0, stream(c), X, mu, vw.ld[i], vw.p[i], B.n, B.rc, B.K, B.z, B.xpart, S.drv.dev);
  }
  CCZ_LAUNCH_CHECK();
}

template <typename T>
void launch_xw(ccz_ctx* c, const GfaState& S, const GfaViews& vw, int i) {
  const GfaBuf& B = S.B;
  const T* X = static_cast<const T*>(vw.X[i]);
  const T* mu = static_cast<const T*>(vw.mu[i]);
  const double* w = B.w + vw.off[i] * B.K;
  double* part = B.xwpart + vw.xwoff[i];
  if (S.K <= GFA_PLAIN_K) {
    const dim3 grid(unsigned((S.n + GFA_SROWS - 1) / GFA_SROWS), unsigned(vw.cs[i]));
    hipLaunchKernelGGL((k_gfa_xw_plain<T>), grid, dim3(256), 0, stream(c), X, mu, vw.ld[i], vw.p[i], B.n, B.K, w, part, S.drv.dev);
  } else {
    const dim3 grid(unsigned((S.n + GFA_XROWS - 1) / GFA_XROWS), unsigned(vw.cs[i]));
    if (S.K <= 16)
      hipLaunchKernelGGL((k_gfa_xw_mfma<T, 1>), grid, dim3(256), 0, stream(c), X, mu, vw.ld[i], vw.p[i], B.n, B.K, w, part, S.drv.dev);
    else
      hipLaunchKernelGGL((k_gfa_xw_mfma<T, 2>), grid, dim3(256), 0, stream(c), X, mu, vw.ld[i], vw.p[i], B.n, B.K, w, part, S.drv.dev);
  }
  CCZ_LAUNCH_CHECK();
}

void enqueue_iteration(ccz_ctx* c, const GfaState& S, const GfaViews& vw) {
  const GfaBuf& B = S.B;
  hipLaunchKernelGGL(k_gfa_covw, dim3(S.M), dim3(256), 0, stream(c), B, S.drv.dev);
  CCZ_LAUNCH_CHECK();
  for (int i = 0; i < S.M; ++i) {
    by_dtype(S.dtype, [&](auto t) { launch_xtz<decltype(t)>(c, S, vw, i); });
    hipLaunchKernelGGL(k_gfa_wfold, dim3(vw.gw[i]), dim3(256), 0, stream(c), B, i, vw.p[i], vw.off[i], S.drv.dev);
    CCZ_LAUNCH_CHECK();
  }
  hipLaunchKernelGGL(k_gfa_covz, dim3(1), dim3(GFA_PT), 0, stream(c), B, vw, S.drv.dev);
  CCZ_LAUNCH_CHECK();
  for (int i = 0; i < S.M; ++i) by_dtype(S.dtype, [&](auto t) { launch_xw<decltype(t)>(c, S, vw, i); });
  hipLaunchKernelGGL(k_gfa_z, dim3(B.gz), dim3(256), 0, stream(c), B, vw, S.drv.dev);
  CCZ_LAUNCH_CHECK();
  hipLaunchKernelGGL(k_gfa_finish, dim3(1), dim3(GFA_PT), 0, stream(c), B, vw, S.drv.dev);
  CCZ_LAUNCH_CHECK();
  const int gc = int(std::max<int64_t>(1, std::min<int64_t>(256, (S.n + B.ptot + 2047) / 2048)));
  hipLaunchKernelGGL(k_gfa_compact, dim3(gc), dim3(256), 0, stream(c), B, S.drv.dev);
  CCZ_LAUNCH_CHECK();
}

// sum fl(x - mu)^2 into *out0 and, when out1, the sum of the ddof = 1 column variances into *out1 (both on the device); `part`
// holds 2 sc p doubles, `cmean` p
template <typename T>
void launch_stats(ccz_ctx* c, const void* X, const void* mu, int64_t ld, int64_t p, int64_t n, int sc, int src, double* part, double* cmean,
                  double* out0, double* out1) {
  const dim3 grid(unsigned((p + 255) / 256), unsigned(sc));
  for (int pass = 0; pass < (out1 ? 2 : 1); ++pass) {
    hipLaunchKernelGGL((k_gfa_stat<T>), grid, dim3(256), 0, stream(c), static_cast<const T*>(X), static_cast<const T*>(mu), ld, p, int(n), src,
                       pass, cmean, part);
    CCZ_LAUNCH_CHECK();
    hipLaunchKernelGGL(k_gfa_stat_fold, dim3(1), dim3(GFA_PT), 0, stream(c), part, sc, p, int(n), pass, cmean, out0, out1);
    CCZ_LAUNCH_CHECK();
  }
}

GfaState* gfa_create(ccz_ctx* c, int dtype, int M, const int64_t* p, int64_t n, int64_t k, double tol, int64_t max_iter, int drop_k,
                     int64_t chunk) {
  check_dtype("gfa", dtype);
  check_view_count("gfa", M, GFA_MAXV);
  if (k < 1 || k > GFA_MAXK) fail(CCZ_EUNSUP, "gfa: 1 to %d latent dimensions are supported, got %lld", GFA_MAXK, (long long)k);
  if (!p || n < 2 || n > (int64_t(1) << 30) || max_iter < 1 || max_iter > (int64_t(1) << 30) || chunk < 1 || !(tol >= 0.0))
    fail(CCZ_EINVAL, "gfa: bad argument");
  check_no_empty_view("gfa", M, p);
  return new_state<GfaState>(c, [&](GfaState& S) {
    S.dtype = dtype; S.M = M; S.n = n; S.K = k; S.chunk = chunk;
    S.p.assign(p, p + M);
    GfaBuf& B = S.B;
    memset(&B, 0, sizeof(B));
    memset(&S.shape, 0, sizeof(S.shape));
    B.n = int(n); B.M = M; B.K = int(k); B.tol = tol; B.max_iter = int(max_iter); B.drop_k = drop_k ? 1 : 0;
    const bool plain = k <= GFA_PLAIN_K;
    int64_t xwtot = 0;
    for (int i = 0; i < M; ++i) {
      GfaViews& sh = S.shape;
      sh.p[i] = p[i];
      sh.off[i] = B.ptot;
      B.ptot += p[i];
      B.pmax = std::max(B.pmax, p[i]);
      sh.cs[i] = column_splits(n, plain ? GFA_SROWS : GFA_XROWS, p[i], GFA_CSMAX);
      sh.xwoff[i] = xwtot;
      xwtot += int64_t(sh.cs[i]) * n * k;
      sh.gw[i] = int(std::max<int64_t>(1, std::min<int64_t>(GFA_G, (p[i] + GFA_FB - 1) / GFA_FB)));
    }
    // the X'z partials are nchunk x pmax x k doubles: as many row chunks as the scratch budget holds, 64 at most, of >= 64 rows
    row_chunks(n, std::min<int64_t>(64, GFA_SCRATCH_BYTES / (B.pmax * k * 8)), &B.nchunk, &B.rc);
    B.gz = int(std::max<int64_t>(1, std::min<int64_t>(GFA_G, (n + GFA_ZR - 1) / GFA_ZR)));
    // the setup pass keeps 2 sc pmax partials in the same scratch
    row_chunks(n, int64_t(B.nchunk) * k / 2, &B.sc, &B.src);
    B.z = S.get(c, size_t(n) * k);
    B.w = S.get(c, size_t(B.ptot) * k);
    B.xw = S.get(c, size_t(M) * n * k);
    B.xwpart = S.get(c, size_t(xwtot));
    B.xpart = S.get(c, std::max<size_t>(size_t(B.nchunk) * B.pmax * k, size_t(2) * B.sc * B.pmax));
    B.covz = S.get(c, GFA_KK);
    B.zz = S.get(c, GFA_KK);
    B.covw = S.get(c, size_t(M) * GFA_KK);
    B.ww = S.get(c, size_t(M) * GFA_KK);
    B.alpha = S.get(c, size_t(M) * GFA_MAXK);
    B.bard = S.get(c, size_t(M) * GFA_MAXK);
    B.tau = S.get(c, M);
    B.btau = S.get(c, M);
    B.yconst = S.get(c, M);
    B.datavar = S.get(c, M);
    B.wwpart = S.get(c, size_t(M) * GFA_G * GFA_KK);
    B.zpart = S.get(c, size_t(GFA_G) * GFA_ZP);
    B.cmean = S.get(c, size_t(B.pmax));
    S.drv.create(c);
  });
}

void gfa_setup(ccz_ctx* c, GfaState& S, const ccz_view* views, const void* const* means) {
  const GfaViews vw = make_views(S, views, means);
  const GfaBuf& B = S.B;
  for (int i = 0; i < S.M; ++i)
    by_dtype(S.dtype, [&](auto t) {
      launch_stats<decltype(t)>(c, vw.X[i], vw.mu[i], vw.ld[i], vw.p[i], S.n, B.sc, B.src, B.xpart, B.cmean, B.yconst + i, B.datavar + i);
    });
  zero(c, B.w, size_t(B.ptot) * S.K * 8);
  zero(c, B.xw, size_t(S.M) * S.n * S.K * 8);
  hipLaunchKernelGGL(k_gfa_zz0, dim3(B.gz), dim3(256), 0, stream(c), B);
  CCZ_LAUNCH_CHECK();
  hipLaunchKernelGGL(k_gfa_init, dim3(1), dim3(GFA_PT), 0, stream(c), B, vw, S.drv.dev);
  CCZ_LAUNCH_CHECK();
}

GfaStatus read_status(ccz_ctx* c, const GfaState& S) {
  GfaStatus st;
  d2h(c, &st, S.drv.dev, sizeof(st));
  return st;
}

// rows x ka of a device matrix with leading dimension ld, packed, to the host
void fetch(ccz_ctx* c, const double* src, int64_t rows, int64_t ld, int64_t ka, double* out) {
  std::vector<double> tmp(size_t(rows) * ld);
  d2h(c, tmp.data(), src, tmp.size() * 8);
  for (int64_t r = 0; r < rows; ++r)
    for (int64_t a = 0; a < ka; ++a) out[r * ka + a] = tmp[size_t(r) * ld + a];
}

}  // namespace
}  // namespace ccz

extern "C" {

int ccz_gfa_create(ccz_handle h, int dtype, int n_views, const int64_t* p, int64_t n_rows, int64_t k, double tol, int64_t max_iter,
                   int drop_k, int64_t chunk_iters, void** state_out) {
  CCZ_GUARD(h, {
    if (!state_out) ccz::fail(CCZ_EINVAL, "null argument");
    *state_out = nullptr;
    *state_out = ccz::gfa_create(h, dtype, n_views, p, n_rows, k, tol, max_iter, drop_k, chunk_iters);
  })
}

int ccz_gfa_destroy(ccz_handle h, void* state) {
  CCZ_GUARD(h, {
    if (state) ccz::free_state(h, static_cast<ccz::GfaState*>(state));
  })
}

int ccz_gfa_set_init(ccz_handle h, void* state, const double* z0_host) {
  CCZ_GUARD(h, {
    ccz::GfaState& S = *ccz::as_state<ccz::GfaState>("gfa", state);
    if (!z0_host) ccz::fail(CCZ_EINVAL, "gfa: null initial z");
    S.restart(h);
    ccz::h2d(h, S.B.z, z0_host, size_t(S.n) * S.K * 8);
    S.has_init = true;
    S.ready = false;
  })
}

int ccz_gfa_setup(ccz_handle h, void* state, const ccz_view* views, const void* const* means_dev) {
  CCZ_GUARD(h, {
    ccz::GfaState& S = *ccz::as_state<ccz::GfaState>("gfa", state);
    if (!S.has_init) ccz::fail(CCZ_EINVAL, "gfa: ccz_gfa_set_init has not been called");
    ccz::gfa_setup(h, S, views, means_dev);
    S.has_init = false;   // a new fit needs a new z0: the iterations overwrite it
    S.ready = true;
  })
}

int ccz_gfa_iterations(ccz_handle h, void* state, const ccz_view* views, const void* const* means_dev, int64_t n_iters,
                       int64_t* iters_known, int* stopped_known) {
  CCZ_GUARD(h, {
    ccz::GfaState& S = *ccz::as_state<ccz::GfaState>("gfa", state);
    if (!S.ready) ccz::fail(CCZ_EINVAL, "gfa: ccz_gfa_setup has not been called");
    ccz::run_chunk(h, "gfa", "n_iters", S, n_iters, iters_known, stopped_known, &ccz::GfaStatus::iters,
                   [&] { return ccz::make_views(S, views, means_dev); },
                   [&](const ccz::GfaViews& vw, int64_t) { ccz::enqueue_iteration(h, S, vw); });
  })
}

int ccz_gfa_status(ccz_handle h, void* state, int64_t* iters, int* stopped, int* k_active, int* stable, double* rel_change,
                   int* n_prunes, int64_t* prune_iters, int* prune_k) {
  CCZ_GUARD(h, {
    ccz::GfaState& S = *ccz::as_state<ccz::GfaState>("gfa", state);
    if (!S.ready) ccz::fail(CCZ_EINVAL, "gfa: ccz_gfa_setup has not been called");
    const ccz::GfaStatus st = ccz::read_status(h, S);
    if (iters) *iters = st.iters;
    if (stopped) *stopped = st.stopped;
    if (k_active) *k_active = st.k;
    if (stable) *stable = st.stable;
    if (rel_change) *rel_change = st.rel_change;
    if (n_prunes) *n_prunes = st.nprune;
    for (int i = 0; i < st.nprune; ++i) {
      if (prune_iters) prune_iters[i] = st.prune_iter[i];
      if (prune_k) prune_k[i] = st.prune_k[i];
    }
  })
}

int ccz_gfa_peek(ccz_handle h, void* state, int what, int view, double* out_host) {
  CCZ_GUARD(h, {
    ccz::GfaState& S = *ccz::as_state<ccz::GfaState>("gfa", state);
    const ccz::GfaBuf& B = S.B;
    if (!S.ready) ccz::fail(CCZ_EINVAL, "gfa: ccz_gfa_setup has not been called");
    if (!out_host || view < 0 || view >= S.M) ccz::fail(CCZ_EINVAL, "gfa: bad argument");
    const int64_t ka = ccz::read_status(h, S).k, n = S.n, K = S.K, p = S.p[view], KS = ccz::GFA_MAXK, KK = ccz::GFA_KK;
    switch (what) {
      case CCZ_GFA_PEEK_Z: ccz::fetch(h, B.z, n, K, ka, out_host); break;
      case CCZ_GFA_PEEK_W: ccz::fetch(h, B.w + S.shape.off[view] * K, p, K, ka, out_host); break;
      case CCZ_GFA_PEEK_XW: ccz::fetch(h, B.xw + int64_t(view) * n * K, n, K, ka, out_host); break;
      case CCZ_GFA_PEEK_COV_Z: ccz::fetch(h, B.covz, ka, KS, ka, out_host); break;
      case CCZ_GFA_PEEK_COV_W: ccz::fetch(h, B.covw + view * KK, ka, KS, ka, out_host); break;
      case CCZ_GFA_PEEK_WW: ccz::fetch(h, B.ww + view * KK, ka, KS, ka, out_host); break;
      case CCZ_GFA_PEEK_ZZ: ccz::fetch(h, B.zz, ka, KS, ka, out_host); break;
      case CCZ_GFA_PEEK_ALPHA: ccz::d2h(h, out_host, B.alpha + view * KS, size_t(ka) * 8); break;
      case CCZ_GFA_PEEK_B_ARD: ccz::d2h(h, out_host, B.bard + view * KS, size_t(ka) * 8); break;
      case CCZ_GFA_PEEK_TAU: ccz::d2h(h, out_host, B.tau, size_t(S.M) * 8); break;
      case CCZ_GFA_PEEK_B_TAU: ccz::d2h(h, out_host, B.btau, size_t(S.M) * 8); break;
      case CCZ_GFA_PEEK_SETUP:
        ccz::d2h(h, out_host, B.yconst + view, 8);
        ccz::d2h(h, out_host + 1, B.datavar + view, 8);
        break;
      default: ccz::fail(CCZ_EINVAL, "gfa: unknown buffer %d", what);
    }
  })
}

int ccz_gfa_get_result(ccz_handle h, void* state, int* k_active, double* z_host, double* cov_z_host, double* w_host, double* cov_w_host,
                       double* alpha_host, double* b_ard_host, double* tau_host, double* b_tau_host) {
  CCZ_GUARD(h, {
    ccz::GfaState& S = *ccz::as_state<ccz::GfaState>("gfa", state);
    const ccz::GfaBuf& B = S.B;
    if (!S.ready) ccz::fail(CCZ_EINVAL, "gfa: ccz_gfa_setup has not been called");
    if (!k_active) ccz::fail(CCZ_EINVAL, "null argument");
    const int64_t ka = ccz::read_status(h, S).k, KS = ccz::GFA_MAXK, KK = ccz::GFA_KK;
    *k_active = int(ka);
    if (z_host) ccz::fetch(h, B.z, S.n, S.K, ka, z_host);
    if (cov_z_host) ccz::fetch(h, B.covz, ka, KS, ka, cov_z_host);
    if (w_host) ccz::fetch(h, B.w, B.ptot, S.K, ka, w_host);
    for (int m = 0; m < S.M; ++m) {
      if (cov_w_host) ccz::fetch(h, B.covw + m * KK, ka, KS, ka, cov_w_host + m * ka * ka);
      if (alpha_host) ccz::d2h(h, alpha_host + m * ka, B.alpha + m * KS, size_t(ka) * 8);
      if (b_ard_host) ccz::d2h(h, b_ard_host + m * ka, B.bard + m * KS, size_t(ka) * 8);
    }
    if (tau_host) ccz::d2h(h, tau_host, B.tau, size_t(S.M) * 8);
    if (b_tau_host) ccz::d2h(h, b_tau_host, B.btau, size_t(S.M) * 8);
  })
}

int ccz_gfa_sumsq(ccz_handle h, int dtype, const ccz_view* view, int64_t n_rows, const void* mean_dev, double* sumsq_host) {
  CCZ_GUARD(h, {
    if (!view || !view->data || !sumsq_host || n_rows < 1 || n_rows > (int64_t(1) << 30) || view->cols < 1 || view->ld < view->cols)
      ccz::fail(CCZ_EINVAL, "gfa: bad argument");
    ccz::check_dtype("gfa", dtype);
    int sc, src;
    ccz::row_chunks(n_rows, 64, &sc, &src);
    ccz::DBuf part(h, int64_t(2) * sc * view->cols), cmean(h, view->cols), out(h, 1);
    ccz::by_dtype(dtype, [&](auto t) {
      ccz::launch_stats<decltype(t)>(h, view->data, mean_dev, view->ld, view->cols, n_rows, sc, src, part, cmean, out, nullptr);
    });
    ccz::d2h(h, sumsq_host, out, 8);
  })
}

}  // extern "C"
