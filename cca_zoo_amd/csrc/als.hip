// ALS models with deflation (PLS_ALS / SCCA_PMD / ParkhomenkoCCA / SCCA_Span): whole sweeps on the device.
//
// Reference: cca_zoo/linear/_iterative.py:38-158 (the loop, _target_score), :166-223 (PLS_ALS), :231-380 (SCCA_PMD and its
// bisection), :631-722 (SCCA_Span), :839-930 (ParkhomenkoCCA), cca_zoo/_utils/_linalg.py:76-116 (soft_threshold, deflate).
// The reference rewrites a float64 copy of every view once per latent dimension.  After d dimensions that copy equals
// (I - Q_i Q_i') (X_i - mu_i) with Q_i (n x d) the normalised scores of the earlier dimensions, so here the rows are read
// where they lie, in their own precision, and the two n-vectors of an update are corrected instead:
//   X_d w  = s - Q_i (Q_i' s),  s = (X_i - mu_i) w            k_als_score (raw s) + the correction in the next prologue
//   X_d' t = (X_i - mu_i)' (t - Q_i (Q_i' t))                 k_als_prologue (t~) + k_als_xt
// One sweep, for M views (Gauss-Seidel: view i's new w_i feeds view i + 1's target):
//   M x  k_als_score          first sweep of a dimension only (the scores of the initial vectors); returns at once otherwise
//   per view i:
//     k_als_prologue          one workgroup: t = sum_{j != i} (s_j - Q_j Q_j' s_j), guarded normalisation, t~ = t - Q_i Q_i' t
//     k_als_xt                column strips x row chunks: per-chunk partial sums of (X_i - mu_i)' t~
//     k_als_fold              raw = sum of the chunk partials in chunk order; per-workgroup |raw|_1, max |raw|, sum of squares
//     k_als_levels x 10 / 13  soft-threshold-at-L1 and top-s only: 31 candidate levels per pass over raw (5 halvings of the
//                             bisection / 5 bits of the s-th largest magnitude's bit pattern)
//     k_als_norm              the same two rules: the final level, the sum of squares of the thresholded vector
//     k_als_apply             w_i = rule(raw) (guarded normalisation), per-workgroup partial |w_i - w_i_old|^2
//     k_als_score             s_i = (X_i - mu_i) w_i
//   k_als_finish              one workgroup: delta, the tol / max_iter test; at the end of a dimension the normalised corrected
//                             scores become column d of every Q_i (guarded), the dimension counter advances
//   k_als_advance             at the end of a dimension only: column d of the weights <- w, w <- the next initial vectors
// Every kernel reads the status word first and returns at once when the fit has stopped; the host never waits inside a chunk.
// All reductions run in a fixed order (per-thread strided sums, wave butterflies, waves and workgroups in index order):
// two fits of the same inputs give the same bits.
//
// A view marked sparse (ccz_als_set_sparse, these four rules only) lies in CSR and CSC form and is centred implicitly:
// k_als_score becomes k_als_sparse_dot (mu' w) + k_als_score_csr, k_als_xt becomes k_als_sparse_dot (1' t~) + k_als_xt_csc,
// which writes the one chunk the fold sums; every other kernel of the sweep is unchanged (see "sparse views" below).
//
// SCCA_ADMM (cca_zoo/linear/_iterative.py:388-514) runs on the same buffers with its own ordering (Jacobi in the scores: the
// targets of ALL views come from the vectors the iteration started with) and its own rule.  One iteration:
//   M x  k_als_score          first iteration of a dimension only, as above
//   per view i:
//     k_als_admm_kq/_h or _xtq/_afold, k_als_admm_gnorm, k_als_admm_lfinal
//                             first iteration of a dimension only (return at once otherwise): L_i = |X_d' X_d|_F / n + mu from
//                             the Gram of the centred view, formed once on its smaller side (ccz_als_admm_setup), and Q_i
//     k_als_admm_prologue     one workgroup: r = s_i - t_i, t_i as above, r~ = r - Q_i Q_i' r
//     k_als_xt                per-chunk partial sums of (X_i - mu_i)' r~  =  X_d' X_d w_i - X_d' t_i
//     k_als_admm_fold         w' = w_i - (that + mu eta_i) / L_i into raw; partial sums of squares of soft(w' + eta_i, tau_i / mu)
//     k_als_admm_apply        z_i = that vector, over its norm when the norm exceeds 1; eta_i += w' - z_i; w_i <- z_i;
//                             per-workgroup partial |z_i - w_i|^2
//   M x  k_als_score          s_i = (X_i - mu_i) w_i of the new vectors: the next iteration's targets, the Q columns of k_als_finish
//   k_als_finish, k_als_advance as above
// z_i and w_i coincide between iterations (the reference starts from z = w and ends every iteration with w = z), so w_i - z_i
// in its gradient is exactly zero and z has no buffer of its own; eta_i counts as zero at a dimension's first iteration.
//
// SCCA_IPLS and ElasticCCA (cca_zoo/linear/_iterative.py:522-623, :730-831, :938-982) regress the target on the deflated view
// with an elastic-net penalty.  The reference's solver visits the coordinates in random order; whenever the minimiser is
// unique the outer update does not depend on that order, so here the solve is cyclic coordinate descent on the Gram matrix
// G_i of the deflated view (formed once on the p side, deflated in place by G_i -= a a', a = (X_i - mu_i)' q~_d).  Its length
// depends on the data, so the sweep is cut into UNITS of a fixed kernel sequence and the status word carries where the
// sweep stands (view, phase); every kernel of a unit returns at once unless the status names its view and phase:
//   per view i:
//     phase 0  k_als_enet_prologue (t, t't, t~), k_als_xt, k_als_enet_rinit (q = X_d' t into raw; r = q - G c from the
//              view's previous coefficients c, c = 0 at a dimension's first solve), then phase 1
//     phase 1  up to ENET_CD_CHUNK (16) x [ per block of 64 coordinates: k_als_enet_block (one wave: the 64 sequential steps on the
//              diagonal tile in LDS), k_als_enet_update (r -= G[:, block] delta for the rest of r; returns at once when
//              delta = 0);  k_als_enet_check (scikit-learn's stop rule in Gram form; phase 2 when it holds) ]
//     phase 2  k_als_score of c, k_als_enet_std (SCCA_IPLS: the population standard deviation of the corrected score),
//              k_als_enet_apply (w_i = c or c / std, partial |w_i - w_i_old|^2), then phase 0 of view i + 1
//   k_als_finish (once every view is done), k_als_advance; at the end of a dimension k_als_admm_xtq / _afold and
//   k_als_enet_deflate bring every G_i up to date
// A solve that needs more sweeps than its unit holds goes on in the next unit: all other kernels of the units between pass.
//
// Precision: x - mu is rounded in the views' precision (the reference's own `v - v.mean(0)`), then widened; every product
// and sum is fp64 (the reference's fp64 initial w promotes every product, cca_zoo/linear/_iterative.py:88-89).
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

constexpr int ALS_MAXV = 8;          // views per fit
constexpr int ALS_MAXK = 32;         // latent dimensions per fit
constexpr int ALS_STRIP = 1024;      // k_als_xt: columns per workgroup (256 threads x 4)
constexpr int ALS_SROWS = 4;         // k_als_score: rows per workgroup
constexpr int ALS_MAXG = 128;        // rule kernels: workgroups per p-vector
constexpr int ALS_NC = 31;           // candidate levels per k_als_levels pass
constexpr int ALS_PMD_PASSES = 10;   // 50 halvings, 5 per pass
constexpr int ALS_SPAN_PASSES = 13;  // bits 62..0 of a non-negative double: 12 passes of 5 bits, one of 3

constexpr int ALS_ADMM_MAXSIDE = 16384;   // SCCA_ADMM: largest min(n, p_i), the side of a view's stored Gram
constexpr int ALS_LG = 256;          // k_als_admm_gnorm: workgroups (one partial sum each)
constexpr int ALS_GT = 64;           // k_als_gram: tile edge
constexpr int ALS_GKC = 32;          // k_als_gram: contraction indices per LDS stage
constexpr int ALS_GLD = ALS_GKC + 1; // LDS row stride (doubles)

// Elastic-net solve.  ENET_BW coordinates per block: one wavefront, so the 64 dependent steps of a block run without a
// workgroup barrier (a shuffle hands delta_j to the other lanes) and the diagonal tile, 64 x 64 doubles = 32 KiB, fits the
// LDS one workgroup gets by default; a wider block would pay a barrier per coordinate, which costs more than the launch
// it saves.
constexpr int ENET_BW = 64;
constexpr int ENET_MAXP = ALS_ADMM_MAXSIDE;   // widest view: G_i is p_i x p_i
constexpr int ENET_CAP = 1000;       // CD sweeps per solve (scikit-learn's max_iter)
constexpr int ENET_CD_CHUNK = 16;    // CD sweeps enqueued per view and unit, at most ...
constexpr int ENET_CD_BLOCKS = 64;   // ... and as many as keep it near this many block steps (at least one sweep)

enum { RULE_NORMALISE = 0, RULE_SOFT_FIXED = 1, RULE_SOFT_L1 = 2, RULE_TOP_S = 3, RULE_ADMM = 4, RULE_ENET = 5 };

struct AlsStatus {
  double last_delta[ALS_MAXK];     // delta of the last sweep of each dimension
  long long iters[ALS_MAXK];       // sweeps taken per dimension
  long long total;                 // sweeps applied in all
  int dim;                         // current dimension (== k once stopped)
  int sweep;                       // sweeps done in the current dimension
  int stopped;
  int advance;                     // the last finish ended a dimension (read by k_als_advance)
  // elastic net only (zero otherwise)
  long long inner[ALS_MAXK];       // CD sweeps per dimension
  int view, phase;                 // where the current sweep stands: the view being updated and its phase (0, 1, 2)
  int isweep;                      // CD sweeps done in the current solve
  int capped;                      // solves that ended on ENET_CAP without meeting the stop rule
};

struct AlsViews {
  const void* X[ALS_MAXV];
  const void* mu[ALS_MAXV];
  int64_t ld[ALS_MAXV];
  int64_t p[ALS_MAXV];
  int64_t off[ALS_MAXV];           // offset of view i in the concatenated p-vectors
  int cs[ALS_MAXV];                // column splits of k_als_score
  int ng[ALS_MAXV];                // rule workgroups
  double par[ALS_MAXV];            // rule parameter: tau (soft fixed), the L1 bound (soft at L1), s (top s)
  int rule[ALS_MAXV];              // the rule of this view (top s with s >= p is plain normalisation)
};

// SCCA_ADMM: what ccz_als_admm_setup leaves for view i (side = min(n, p_i); the n side when n <= p_i)
struct AdmmView {
  double* G;        // side x side: (X - mu) (X - mu)' or (X - mu)' (X - mu)
  double* U;        // k x side: n side H = K Q - Q (Q' K Q) / 2 (deflated Gram = K - Q H' - H Q'); p side A = (X - mu)' Q (G - A A')
  double* KQ;       // n side only, k x n: K Q
  int64_t side;
  int nside;
};

// the device buffers of one fit
struct AlsBuf {
  double* w;        // ptot: current vectors
  double* raw;      // ptot
  double* init;     // k x ptot: initial vectors of every dimension
  double* Wout;     // ptot x k row-major: finished columns
  double* spart;    // M x csmax x n: column-split partial scores
  double* Q;        // M x k x n: Q_i column a at (i k + a) n
  double* tt;       // n: corrected, normalised target
  double* xpart;    // nchunk x pmax: row-chunk partial sums of X' t~
  double* fstat;    // M x ALS_MAXG x 3: fold partials (L1, max, sum of squares)
  double* lpart;    // 2 x ALS_MAXG x ALS_NC: level-pass partials (ping-pong by pass parity)
  double* lstate;   // (passes + 1) x 2: bracket after each pass (lo, hi) / (bit prefix, unused)
  double* nstat;    // ALS_MAXG: k_als_norm partial sums of squares
  double* thr;      // M x 2: final level of view i's last update, 1.0 when thresholding applied
  double* dpart;    // M x ALS_MAXG: partial |w - w_old|^2
  double* eta;      // SCCA_ADMM, ptot: scaled dual variables
  double* tt2;      // SCCA_ADMM, n: the view's own corrected score while the prologue forms s_i - t_i
  double* lip;      // SCCA_ADMM, M: L_i of the current dimension
  double* gpart;    // SCCA_ADMM, ALS_LG: partial sums of squares of a deflated Gram
  double* coef;     // elastic net, ptot: the coefficients of every view's last solve
  double* res;      // elastic net, pmax: r = q - G c of the running solve
  double* dl;       // elastic net, ENET_BW: the block's coordinate changes
  double* bstat;    // elastic net, nbmax x 2: per block max |delta|, max |c|
  double* scal;     // elastic net, M x 4: t't, the gap, the score's standard deviation, the sweeps of the last solve
  int enet;         // elastic net: the status carries (view, phase)
  int n, M, k, csmax, nchunk, rc;
  int64_t ptot, pmax;
};

__device__ __forceinline__ double als_soft(double x, double t) {
  const double a = fabs(x) - t;
  return a > 0.0 ? copysign(a, x) : 0.0;
}

// ---- score: column-split partial sums of s = (X - mu) w ----------------------------------------------------------------
// grid (ceil(n / 4), cs), 256 threads: 4 rows x one column range per workgroup, 4 consecutive columns per thread and step.
// first_only: the scores of a dimension's initial vectors -- runs only while no sweep of the dimension is done.
// gate >= 0 (elastic net): runs only in phase 2 of that view.
template <typename T>
__global__ void __launch_bounds__(256) k_als_score(const T* __restrict__ X, const T* __restrict__ mu, int64_t ld, int64_t p, int n,
                                                  const double* __restrict__ w, double* __restrict__ spart, int first_only,
                                                  int gate, const AlsStatus* st) {
  if (fit_stopped(st)) return;
  if (first_only && (st->sweep != 0 || st->view != 0 || st->phase != 0)) return;
  if (gate >= 0 && (st->view != gate || st->phase != 2)) return;
  __shared__ double sh[4];
  const int r0 = blockIdx.x * ALS_SROWS;
  int64_t c0, c1;
  split_range(p, gridDim.y, blockIdx.y, &c0, &c1);
  const bool vec = vec_ok(X, ld, mu);
  const bool wvec = reinterpret_cast<uintptr_t>(w) % 16 == 0;
  double acc[ALS_SROWS] = {0.0, 0.0, 0.0, 0.0};
  const T* rowp[ALS_SROWS];
  bool live[ALS_SROWS];
#pragma unroll
  for (int t = 0; t < ALS_SROWS; ++t) {
    live[t] = r0 + t < n;
    rowp[t] = X + int64_t(live[t] ? r0 + t : 0) * ld;
  }
#pragma unroll 2
  for (int64_t f0 = c0 + 4 * threadIdx.x; f0 < c1; f0 += 1024) {
    double wv[4];
    T m[4] = {T(0), T(0), T(0), T(0)};
    load4<double>(w, f0, c1, wvec, wv);
    if (mu) load4<T>(mu, f0, c1, vec, m);
#pragma unroll
    for (int t = 0; t < ALS_SROWS; ++t) {
      if (!live[t]) continue;
      T x[4];
      load4<T>(rowp[t], f0, c1, vec, x);
#pragma unroll
      for (int q = 0; q < 4; ++q) acc[t] += double(T(x[q] - m[q])) * wv[q];
    }
  }
#pragma unroll
  for (int t = 0; t < ALS_SROWS; ++t) {
    const double s = block_sum<4>(acc[t], sh);
    if (threadIdx.x == 0 && live[t]) spart[int64_t(blockIdx.y) * n + r0 + t] = s;
  }
}

// ---- the one-workgroup kernels: prologue and finish ------------------------------------------------------------------
constexpr int ALS_PT = 1024;   // threads of the one-workgroup kernels

// dst[r] (+)= s_j[r] - (Q_j Q_j' s_j)[r] over all rows, s_j = the sum of view j's column-split partials, d columns of Q_j
__device__ void als_corrected_score(const AlsBuf& B, const AlsViews& vw, int j, int d, double* dst, bool accumulate, double* coef,
                                    double* sh) {
  const int n = B.n, cs = vw.cs[j];
  const double* sp = B.spart + int64_t(j) * B.csmax * n;
  const double* Q = B.Q + int64_t(j) * B.k * n;
  for (int a = 0; a < d; ++a) {
    double acc = 0.0;
    for (int r = threadIdx.x; r < n; r += ALS_PT) {
      double s = 0.0;
      for (int c = 0; c < cs; ++c) s += sp[int64_t(c) * n + r];
      acc += Q[int64_t(a) * n + r] * s;
    }
    const double c = block_sum<ALS_PT / 64>(acc, sh);
    if (threadIdx.x == 0) coef[a] = c;
  }
  __syncthreads();
  for (int r = threadIdx.x; r < n; r += ALS_PT) {
    double s = 0.0;
    for (int c = 0; c < cs; ++c) s += sp[int64_t(c) * n + r];
    double corr = 0.0;
    for (int a = 0; a < d; ++a) corr += Q[int64_t(a) * n + r] * coef[a];
    dst[r] = (accumulate ? dst[r] : 0.0) + (s - corr);
  }
  __syncthreads();
}

// B.tt = t of view i: the sum of the other views' corrected scores, over its norm when that exceeds 1e-12
// (cca_zoo/linear/_iterative.py:138-158 on the deflated views)
__device__ void als_target(const AlsBuf& B, const AlsViews& vw, int i, int d, double* coef, double* sh) {
  const int n = B.n;
  bool first = true;
  for (int j = 0; j < B.M; ++j) {
    if (j == i) continue;                // i = -1 (ElasticCCA): every view
    als_corrected_score(B, vw, j, d, B.tt, !first, coef, sh);
    first = false;
  }
  if (first) {                           // a single view has no target
    for (int r = threadIdx.x; r < n; r += ALS_PT) B.tt[r] = 0.0;
    __syncthreads();
  }
  double acc = 0.0;
  for (int r = threadIdx.x; r < n; r += ALS_PT) acc += B.tt[r] * B.tt[r];
  const double nrm = sqrt(block_sum<ALS_PT / 64>(acc, sh));
  if (nrm > 1e-12)
    for (int r = threadIdx.x; r < n; r += ALS_PT) B.tt[r] /= nrm;     // every thread rereads only its own rows afterwards
}

// B.tt -= Q_i (Q_i' B.tt); every thread has written only its own rows of B.tt
__device__ void als_correct_target(const AlsBuf& B, int i, int d, double* coef, double* sh) {
  const int n = B.n;
  const double* Q = B.Q + int64_t(i) * B.k * n;
  for (int a = 0; a < d; ++a) {
    double q = 0.0;
    for (int r = threadIdx.x; r < n; r += ALS_PT) q += Q[int64_t(a) * n + r] * B.tt[r];
    const double c = block_sum<ALS_PT / 64>(q, sh);
    if (threadIdx.x == 0) coef[a] = c;
  }
  __syncthreads();
  for (int r = threadIdx.x; r < n; r += ALS_PT) {
    double corr = 0.0;
    for (int a = 0; a < d; ++a) corr += Q[int64_t(a) * n + r] * coef[a];
    B.tt[r] -= corr;
  }
}

// t~ of view i into B.tt
__global__ void __launch_bounds__(ALS_PT) k_als_prologue(AlsBuf B, AlsViews vw, int i, const AlsStatus* st) {
  if (fit_stopped(st)) return;
  __shared__ double sh[ALS_PT / 64];
  __shared__ double coef[ALS_MAXK];
  const int d = st->dim;
  als_target(B, vw, i, d, coef, sh);
  als_correct_target(B, i, d, coef, sh);
}

// SCCA_ADMM: r~ = (s_i - t_i) - Q_i Q_i' (s_i - t_i) into B.tt, so that (X_i - mu_i)' r~ = X_d' X_d w_i - X_d' t_i
// (cca_zoo/linear/_iterative.py:475-480); the scores are those the iteration started with for every view
__global__ void __launch_bounds__(ALS_PT) k_als_admm_prologue(AlsBuf B, AlsViews vw, int i, const AlsStatus* st) {
  if (fit_stopped(st)) return;
  __shared__ double sh[ALS_PT / 64];
  __shared__ double coef[ALS_MAXK];
  const int n = B.n, d = st->dim;
  als_target(B, vw, i, d, coef, sh);
  als_corrected_score(B, vw, i, d, B.tt2, false, coef, sh);
  for (int r = threadIdx.x; r < n; r += ALS_PT) B.tt[r] = B.tt2[r] - B.tt[r];
  als_correct_target(B, i, d, coef, sh);
}

// once per sweep: delta, the stop test, the end of a dimension (cca_zoo/linear/_iterative.py:109-117, :91-93, _linalg.py:108-116)
__global__ void __launch_bounds__(ALS_PT) k_als_finish(AlsBuf B, AlsViews vw, double tol, int max_iter, AlsStatus* st) {
  if (fit_stopped(st) || (B.enet && st->view != B.M)) {     // elastic net: a view's solve is still running
    if (threadIdx.x == 0) st->advance = 0;
    return;
  }
  __shared__ double sh[ALS_PT / 64];
  __shared__ double coef[ALS_MAXK];
  __shared__ int end_dim;
  const int n = B.n, d = st->dim;
  double delta = 0.0;
  for (int i = 0; i < B.M; ++i) {
    const double s = block_sum<ALS_PT / 64>(int(threadIdx.x) < vw.ng[i] ? B.dpart[i * ALS_MAXG + threadIdx.x] : 0.0, sh);
    const double di = sqrt(s);
    if (di > delta) delta = di;             // Python's max(): a NaN after the first entry never wins ...
    if (i == 0 && di != di) delta = di;     // ... and a NaN first entry always does
  }
  if (threadIdx.x == 0) {
    const int sweep = st->sweep + 1;
    st->total += 1;
    st->last_delta[d] = delta;
    st->iters[d] = sweep;
    end_dim = (delta < tol || sweep >= max_iter) ? 1 : 0;
    st->sweep = end_dim ? 0 : sweep;
    st->advance = end_dim;
    st->view = 0;
    st->phase = 0;
  }
  __syncthreads();
  if (!end_dim) return;
  // column d of every Q_i: the corrected score over its norm when |s|^2 > 1e-12, else zeros (no deflation)
  for (int i = 0; i < B.M; ++i) {
    double* q = B.Q + (int64_t(i) * B.k + d) * n;
    als_corrected_score(B, vw, i, d, q, false, coef, sh);
    double acc = 0.0;
    for (int r = threadIdx.x; r < n; r += ALS_PT) acc += q[r] * q[r];
    const double ns = block_sum<ALS_PT / 64>(acc, sh);
    const double nrm = sqrt(ns);
    for (int r = threadIdx.x; r < n; r += ALS_PT) q[r] = ns > 1e-12 ? q[r] / nrm : 0.0;
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    st->dim = d + 1;
    if (d + 1 >= B.k) st->stopped = 1;
  }
}

// at the end of a dimension: Wout[:, dim - 1] <- w, w <- init[dim]
__global__ void __launch_bounds__(256) k_als_advance(AlsBuf B, const AlsStatus* st) {
  if (!st->advance) return;
  const int d = st->dim - 1;
  for (int64_t f = int64_t(blockIdx.x) * 256 + threadIdx.x; f < B.ptot; f += int64_t(gridDim.x) * 256) {
    B.Wout[f * B.k + d] = B.w[f];
    if (d + 1 < B.k) B.w[f] = B.init[int64_t(d + 1) * B.ptot + f];
  }
}

// ---- xt: per-chunk partial sums of (X - mu)' t~ ------------------------------------------------------------------------
// grid (ceil(p / 1024), nchunk), 256 threads: thread t owns columns 1024 bx + 4 t .. + 3 over rows [rc by, rc (by + 1))
template <typename T>
__global__ void __launch_bounds__(256) k_als_xt(const T* __restrict__ X, const T* __restrict__ mu, int64_t ld, int64_t p, int n, int rc,
                                               const double* __restrict__ tt, double* __restrict__ xpart, int gate, const AlsStatus* st) {
  if (fit_stopped(st)) return;
  if (gate >= 0 && (st->view != gate || st->phase != 0)) return;     // elastic net: phase 0 of that view only
  const int64_t f0 = int64_t(blockIdx.x) * ALS_STRIP + 4 * threadIdx.x;
  if (f0 >= p) return;
  const int r0 = blockIdx.y * rc, r1 = min(n, r0 + rc);
  const bool vec = vec_ok(X, ld, mu);
  T m[4] = {T(0), T(0), T(0), T(0)};
  if (mu) load4<T>(mu, f0, p, vec, m);
  double acc[4] = {0.0, 0.0, 0.0, 0.0};
#pragma unroll 4
  for (int r = r0; r < r1; ++r) {
    T x[4];
    load4<T>(X + int64_t(r) * ld, f0, p, vec, x);
    const double t = tt[r];
#pragma unroll
    for (int q = 0; q < 4; ++q) acc[q] += double(T(x[q] - m[q])) * t;
  }
  double* out = xpart + int64_t(blockIdx.y) * p;
#pragma unroll
  for (int q = 0; q < 4; ++q)
    if (f0 + q < p) out[f0 + q] = acc[q];
}

// ---- the rule -------------------------------------------------------------------------------------------------------
// raw = the chunk partials summed in chunk order; per-workgroup (|raw|_1, max |raw|, sum of squares of raw -- of
// soft(raw, tau) for the fixed soft threshold)
__global__ void __launch_bounds__(256) k_als_fold(const double* __restrict__ xpart, int nchunk, int64_t p, double* __restrict__ raw,
                                                 int rule, double par, double* __restrict__ fstat, const AlsStatus* st) {
  if (fit_stopped(st)) return;
  __shared__ double sh[4];
  double l1 = 0.0, mx = 0.0, ss = 0.0;
  for (int64_t f = int64_t(blockIdx.x) * 256 + threadIdx.x; f < p; f += int64_t(gridDim.x) * 256) {
    double v = 0.0;
    for (int c = 0; c < nchunk; ++c) v += xpart[int64_t(c) * p + f];
    raw[f] = v;
    const double a = fabs(v);
    l1 += a;
    mx = fmax(mx, a);
    const double u = rule == RULE_SOFT_FIXED ? als_soft(v, par) : v;
    ss += u * u;
  }
  l1 = block_sum<4>(l1, sh);
  mx = block_max<4>(mx, sh);
  ss = block_sum<4>(ss, sh);
  if (threadIdx.x == 0) {
    fstat[3 * blockIdx.x + 0] = l1;
    fstat[3 * blockIdx.x + 1] = mx;
    fstat[3 * blockIdx.x + 2] = ss;
  }
}

// the fold statistics of one view over its ng <= 256 workgroups, by a whole workgroup of 256 threads (fixed order: one
// partial per thread, wave butterflies, waves in index order); every thread gets the result
__device__ __forceinline__ void als_fold_totals(const double* fstat, int ng, double* l1, double* mx, double* ss, double* sh) {
  const int t = threadIdx.x;
  *l1 = block_sum<4>(t < ng ? fstat[3 * t + 0] : 0.0, sh);
  *mx = block_max<4>(t < ng ? fstat[3 * t + 1] : 0.0, sh);
  *ss = block_sum<4>(t < ng ? fstat[3 * t + 2] : 0.0, sh);
}

// the sums of the previous level pass's partials over the workgroups in index order: thread c < 31 owns candidate c
__device__ __forceinline__ void als_level_totals(const double* lpart, int pass, int ng, double* tot) {
  if (pass > 0 && threadIdx.x < ALS_NC) {
    const double* prev = lpart + size_t((pass - 1) & 1) * ALS_MAXG * ALS_NC;
    double s = 0.0;
    for (int g = 0; g < ng; ++g) s += prev[g * ALS_NC + threadIdx.x];
    tot[threadIdx.x] = s;
  }
  __syncthreads();
}

// The bracket after `pass` passes, by thread 0 of every workgroup (all compute the same bits): from the bracket after
// pass - 1 (lstate) and the sums `tot` of pass - 1's partials (als_level_totals).  Soft at L1 (cca_zoo/linear/_iterative.py:245-253): five halvings
// walk the heap of 31 mids, lo = mid when |soft(raw, mid)|_1 > bound, else hi = mid.  Top s: the largest 5-bit digit v whose
// candidate prefix | v << shift still has at least s magnitudes at or above it.
__device__ void als_bracket(int rule, int pass, double par, double mx, const double* lstate, const double* tot, double* lo,
                            double* hi) {
  if (pass == 0) {
    *lo = 0.0;
    *hi = rule == RULE_SOFT_L1 ? mx : 0.0;
    return;
  }
  double l = lstate[2 * (pass - 1)], h = lstate[2 * (pass - 1) + 1];
  if (rule == RULE_SOFT_L1) {
    int node = 1;
    for (int lev = 0; lev < 5; ++lev) {
      const double mid = (l + h) / 2.0;
      if (tot[node - 1] > par) { l = mid; node = 2 * node + 1; }
      else { h = mid; node = 2 * node; }
    }
  } else {
    const int shift = pass - 1 < 12 ? 58 - 5 * (pass - 1) : 0;
    const int nv = pass - 1 < 12 ? 31 : 7;
    unsigned long long pre = (unsigned long long)__double_as_longlong(l);
    int best = 0;
    for (int v = 1; v <= nv; ++v)
      if (tot[v - 1] >= par) best = v;
    pre |= (unsigned long long)best << shift;
    l = __longlong_as_double((long long)pre);
  }
  *lo = l;
  *hi = h;
}

// the 31 candidate levels of pass `pass` from the bracket (lo, hi)
__device__ void als_candidates(int rule, int pass, double lo, double hi, double* cand) {
  if (rule == RULE_SOFT_L1) {
    double l[ALS_NC + 1], h[ALS_NC + 1];
    l[1] = lo; h[1] = hi;
    for (int node = 1; node <= ALS_NC; ++node) {
      const double mid = (l[node] + h[node]) / 2.0;
      cand[node - 1] = mid;
      if (2 * node + 1 <= ALS_NC) {
        l[2 * node] = l[node]; h[2 * node] = mid;          // |soft|_1 <= bound: hi = mid
        l[2 * node + 1] = mid; h[2 * node + 1] = h[node];  // |soft|_1 >  bound: lo = mid
      }
    }
  } else {
    const int shift = pass < 12 ? 58 - 5 * pass : 0;
    const int nv = pass < 12 ? 31 : 7;
    const unsigned long long pre = (unsigned long long)__double_as_longlong(lo);
    for (int v = 1; v <= ALS_NC; ++v)
      cand[v - 1] = v <= nv ? __longlong_as_double((long long)(pre | ((unsigned long long)v << shift))) : INFINITY;
  }
}

// one pass over raw against 31 levels: sum_f max(|raw_f| - level, 0) (soft at L1) or the count of |raw_f| >= level (top s)
__global__ void __launch_bounds__(256) k_als_levels(const double* __restrict__ raw, int64_t p, int rule, double par, int pass,
                                                   const double* __restrict__ fstat, int ng, double* __restrict__ lstate,
                                                   double* __restrict__ lpart, const AlsStatus* st) {
  if (fit_stopped(st)) return;
  __shared__ double cand[ALS_NC];
  __shared__ double tot[ALS_NC];
  __shared__ double red[4][ALS_NC];
  __shared__ double sh[4];
  __shared__ int skip;
  double l1, mx, ss;
  als_fold_totals(fstat, ng, &l1, &mx, &ss, sh);
  als_level_totals(lpart, pass, ng, tot);
  if (threadIdx.x == 0) {
    skip = (rule == RULE_SOFT_L1 && l1 <= par) ? 1 : 0;     // within the bound: no thresholding (:243-244)
    if (!skip) {
      double lo, hi;
      als_bracket(rule, pass, par, mx, lstate, tot, &lo, &hi);
      if (blockIdx.x == 0) {
        lstate[2 * pass] = lo;
        lstate[2 * pass + 1] = hi;
      }
      als_candidates(rule, pass, lo, hi, cand);
    }
  }
  __syncthreads();
  if (skip) return;
  double lev[ALS_NC], acc[ALS_NC];
#pragma unroll
  for (int c = 0; c < ALS_NC; ++c) { lev[c] = cand[c]; acc[c] = 0.0; }
  for (int64_t f = int64_t(blockIdx.x) * 256 + threadIdx.x; f < p; f += int64_t(gridDim.x) * 256) {
    const double a = fabs(raw[f]);
    if (rule == RULE_SOFT_L1) {
#pragma unroll
      for (int c = 0; c < ALS_NC; ++c) acc[c] += fmax(a - lev[c], 0.0);
    } else {
#pragma unroll
      for (int c = 0; c < ALS_NC; ++c) acc[c] += a >= lev[c] ? 1.0 : 0.0;
    }
  }
#pragma unroll
  for (int c = 0; c < ALS_NC; ++c) {
    const double s = wave_sum(acc[c]);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6][c] = s;
  }
  __syncthreads();
  if (threadIdx.x < ALS_NC)
    lpart[(size_t(pass & 1) * ALS_MAXG + blockIdx.x) * ALS_NC + threadIdx.x] =
        red[0][threadIdx.x] + red[1][threadIdx.x] + red[2][threadIdx.x] + red[3][threadIdx.x];
}

// the final level -- (lo + hi) / 2 after 50 halvings (:254), the s-th largest magnitude -- and the partial sums of squares of
// the thresholded vector
__global__ void __launch_bounds__(256) k_als_norm(const double* __restrict__ raw, int64_t p, int rule, double par, int passes,
                                                 const double* __restrict__ fstat, int ng, const double* __restrict__ lstate,
                                                 const double* __restrict__ lpart, double* __restrict__ thr,
                                                 double* __restrict__ nstat, const AlsStatus* st) {
  if (fit_stopped(st)) return;
  __shared__ double sh[4];
  __shared__ double tot[ALS_NC];
  __shared__ double level;
  __shared__ int skip;
  double l1, mx, ss0;
  als_fold_totals(fstat, ng, &l1, &mx, &ss0, sh);
  als_level_totals(lpart, passes, ng, tot);
  if (threadIdx.x == 0) {
    skip = (rule == RULE_SOFT_L1 && l1 <= par) ? 1 : 0;
    double lv = 0.0;
    if (!skip) {
      double lo, hi;
      als_bracket(rule, passes, par, mx, lstate, tot, &lo, &hi);
      lv = rule == RULE_SOFT_L1 ? (lo + hi) / 2.0 : lo;
    }
    level = lv;
    if (blockIdx.x == 0) {
      thr[0] = lv;
      thr[1] = skip ? 0.0 : 1.0;
    }
  }
  __syncthreads();
  if (skip) return;
  const double lv = level;
  double ss = 0.0;
  for (int64_t f = int64_t(blockIdx.x) * 256 + threadIdx.x; f < p; f += int64_t(gridDim.x) * 256) {
    const double v = raw[f];
    const double u = rule == RULE_SOFT_L1 ? als_soft(v, lv) : (fabs(v) >= lv ? v : 0.0);
    ss += u * u;
  }
  ss = block_sum<4>(ss, sh);
  if (threadIdx.x == 0) nstat[blockIdx.x] = ss;
}

// w = rule(raw), normalised when its norm exceeds 1e-12 (the unthresholded branch of soft at L1 divides unguarded, :244);
// per-workgroup partial |w - w_old|^2
__global__ void __launch_bounds__(256) k_als_apply(const double* __restrict__ raw, int64_t p, int rule, double par,
                                                  const double* __restrict__ fstat, int ng, const double* __restrict__ thr,
                                                  const double* __restrict__ nstat, double* __restrict__ w, double* __restrict__ dpart,
                                                  const AlsStatus* st) {
  if (fit_stopped(st)) return;
  __shared__ double sh[4];
  double l1, mx, ss;
  als_fold_totals(fstat, ng, &l1, &mx, &ss, sh);
  const bool levels = rule == RULE_SOFT_L1 || rule == RULE_TOP_S;
  const bool thresholded = levels && thr[1] != 0.0;
  double lv = 0.0;
  if (thresholded) {                     // uniform over the workgroup
    lv = thr[0];
    ss = block_sum<4>(int(threadIdx.x) < ng ? nstat[threadIdx.x] : 0.0, sh);
  } else if (rule == RULE_SOFT_FIXED) {
    lv = par;
  }
  const double nrm = sqrt(ss);
  const bool divide = (rule == RULE_SOFT_L1 && !thresholded) || nrm > 1e-12;
  double dd = 0.0;
  for (int64_t f = int64_t(blockIdx.x) * 256 + threadIdx.x; f < p; f += int64_t(gridDim.x) * 256) {
    const double v = raw[f];
    double u = v;
    if (rule == RULE_SOFT_FIXED || (rule == RULE_SOFT_L1 && thresholded)) u = als_soft(v, lv);
    else if (rule == RULE_TOP_S && thresholded) u = fabs(v) >= lv ? v : 0.0;
    if (divide) u /= nrm;
    const double diff = u - w[f];
    dd += diff * diff;
    w[f] = u;
  }
  dd = block_sum<4>(dd, sh);
  if (threadIdx.x == 0) dpart[blockIdx.x] = dd;
}

// ---- SCCA_ADMM: the rule ------------------------------------------------------------------------------------------------
// w' = w - (X_d'X_d w - X_d' t + mu (w - z + eta)) / L with w - z = 0 (see the head of the file) into raw; per-workgroup
// partial sums of squares of soft(w' + eta, thr), thr = tau / mu (cca_zoo/linear/_iterative.py:480-483)
__global__ void __launch_bounds__(256) k_als_admm_fold(const double* __restrict__ xpart, int nchunk, int64_t p,
                                                      const double* __restrict__ w, const double* __restrict__ eta,
                                                      const double* __restrict__ lip, double mu, double thr,
                                                      double* __restrict__ raw, double* __restrict__ fstat, const AlsStatus* st) {
  if (fit_stopped(st)) return;
  __shared__ double sh[4];
  const bool first = st->sweep == 0;     // eta = 0 at the start of a dimension
  const double L = *lip;
  double ss = 0.0;
  for (int64_t f = int64_t(blockIdx.x) * 256 + threadIdx.x; f < p; f += int64_t(gridDim.x) * 256) {
    double v = 0.0;
    for (int c = 0; c < nchunk; ++c) v += xpart[int64_t(c) * p + f];
    const double e = first ? 0.0 : eta[f];
    const double wp = w[f] - (v + mu * e) / L;
    raw[f] = wp;
    const double u = als_soft(wp + e, thr);
    ss += u * u;
  }
  ss = block_sum<4>(ss, sh);
  if (threadIdx.x == 0) fstat[3 * blockIdx.x + 2] = ss;
}

// z = soft(w' + eta, thr), over its norm when the norm exceeds 1; eta += w' - z; w <- z; per-workgroup partial |z - w|^2
// (cca_zoo/linear/_iterative.py:483-493)
__global__ void __launch_bounds__(256) k_als_admm_apply(const double* __restrict__ raw, int64_t p, double thr,
                                                       const double* __restrict__ fstat, int ng, double* __restrict__ w,
                                                       double* __restrict__ eta, double* __restrict__ dpart, const AlsStatus* st) {
  if (fit_stopped(st)) return;
  __shared__ double sh[4];
  const bool first = st->sweep == 0;
  const double nrm = sqrt(block_sum<4>(int(threadIdx.x) < ng ? fstat[3 * threadIdx.x + 2] : 0.0, sh));
  double dd = 0.0;
  for (int64_t f = int64_t(blockIdx.x) * 256 + threadIdx.x; f < p; f += int64_t(gridDim.x) * 256) {
    const double e = first ? 0.0 : eta[f], wp = raw[f];
    double z = als_soft(wp + e, thr);
    if (nrm > 1.0) z /= nrm;
    eta[f] = e + wp - z;
    const double diff = z - w[f];
    dd += diff * diff;
    w[f] = z;
  }
  dd = block_sum<4>(dd, sh);
  if (threadIdx.x == 0) dpart[blockIdx.x] = dd;
}

// ---- SCCA_ADMM: L_i = |X_d' X_d|_F / n + mu without the deflated view ---------------------------------------------------
// |X_d' X_d|_F = |X_d X_d'|_F, and with Xc = X - mu, P = I - Q Q':  X_d X_d' = P K P (K = Xc Xc'),  X_d' X_d = G - A A'
// (G = Xc' Xc, A = Xc' Q).  The Gram of the smaller side is formed once (k_als_gram); at the first iteration of a dimension
// the kernels below bring K Q / A up to date with the newest column of Q and sum the squares of the deflated entries.  They
// return at once on every other iteration.
__device__ __forceinline__ bool admm_not_first(const AlsStatus* st) { return fit_stopped(st) || st->sweep != 0; }
// elastic net: the newest column of A is taken right after the finish that ended a dimension
__device__ __forceinline__ bool acol_off(const AlsStatus* st, int enet) {
  return enet ? (fit_stopped(st) || !st->advance) : (admm_not_first(st) || st->dim == 0);
}

// n side: column d - 1 of K Q, one wave per row of K
__global__ void __launch_bounds__(256) k_als_admm_kq(const double* __restrict__ K, int n, const double* __restrict__ Q,
                                                    double* __restrict__ KQ, const AlsStatus* st) {
  if (admm_not_first(st) || st->dim == 0) return;
  const int a = st->dim - 1, r = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (r >= n) return;
  const double* q = Q + int64_t(a) * n;
  double s = 0.0;
  for (int c = threadIdx.x & 63; c < n; c += 64) s += K[int64_t(r) * n + c] * q[c];
  s = wave_sum(s);
  if ((threadIdx.x & 63) == 0) KQ[int64_t(a) * n + r] = s;
}

// n side: H = K Q - Q (Q' K Q) / 2 over the d columns in use, one workgroup
__global__ void __launch_bounds__(ALS_PT) k_als_admm_h(int n, const double* __restrict__ Q, const double* __restrict__ KQ,
                                                      double* __restrict__ H, const AlsStatus* st) {
  if (admm_not_first(st) || st->dim == 0) return;
  __shared__ double sh[ALS_PT / 64];
  __shared__ double Cm[ALS_MAXK * ALS_MAXK];
  const int d = st->dim;
  for (int a = 0; a < d; ++a)
    for (int b = 0; b < d; ++b) {
      double acc = 0.0;
      for (int r = threadIdx.x; r < n; r += ALS_PT) acc += Q[int64_t(a) * n + r] * KQ[int64_t(b) * n + r];
      const double c = block_sum<ALS_PT / 64>(acc, sh);
      if (threadIdx.x == 0) Cm[a * ALS_MAXK + b] = c;
    }
  __syncthreads();
  for (int r = threadIdx.x; r < n; r += ALS_PT)
    for (int a = 0; a < d; ++a) {
      double qc = 0.0;
      for (int b = 0; b < d; ++b) qc += Q[int64_t(b) * n + r] * Cm[b * ALS_MAXK + a];
      H[int64_t(a) * n + r] = KQ[int64_t(a) * n + r] - 0.5 * qc;
    }
}

// p side: per-chunk partial sums of column d - 1 of A = (X - mu)' Q, one thread per column of X
template <typename T>
__global__ void __launch_bounds__(256) k_als_admm_xtq(const T* __restrict__ X, const T* __restrict__ mu, int64_t ld, int64_t p, int n,
                                                     int rc, const double* __restrict__ Q, double* __restrict__ xpart,
                                                     int enet, const AlsStatus* st) {
  if (acol_off(st, enet)) return;
  const int64_t f = int64_t(blockIdx.x) * 256 + threadIdx.x;
  if (f >= p) return;
  const double* q = Q + int64_t(st->dim - 1) * n;
  const int r0 = blockIdx.y * rc, r1 = min(n, r0 + rc);
  const T m = mu ? mu[f] : T(0);
  double acc = 0.0;
  for (int r = r0; r < r1; ++r) acc += double(T(X[int64_t(r) * ld + f] - m)) * q[r];
  xpart[int64_t(blockIdx.y) * p + f] = acc;
}

// p side: column d - 1 of A = the chunk partials summed in chunk order
__global__ void __launch_bounds__(256) k_als_admm_afold(const double* __restrict__ xpart, int nchunk, int64_t p,
                                                       double* __restrict__ A, int enet, const AlsStatus* st) {
  if (acol_off(st, enet)) return;
  const int64_t f = int64_t(blockIdx.x) * 256 + threadIdx.x;
  if (f >= p) return;
  double v = 0.0;
  for (int c = 0; c < nchunk; ++c) v += xpart[int64_t(c) * p + f];
  A[int64_t(st->dim - 1) * p + f] = v;
}

// per-workgroup partial sums of squares of the deflated Gram, entry by entry (expanding the norm instead would cancel):
// n side G[r][c] - sum_a (Q[a][r] H[a][c] + H[a][r] Q[a][c]), p side G[r][c] - sum_a A[a][r] A[a][c].  Workgroup b takes
// rows b, b + gridDim.x, ...; U = H or A, Qn = Q of the n side
__global__ void __launch_bounds__(256) k_als_admm_gnorm(const double* __restrict__ G, int64_t side, const double* __restrict__ U,
                                                       const double* __restrict__ Qn, int nside, double* __restrict__ gpart,
                                                       const AlsStatus* st) {
  if (admm_not_first(st)) return;
  __shared__ double sh[4];
  __shared__ double ur[ALS_MAXK], qr[ALS_MAXK];
  const int d = st->dim;
  double acc = 0.0;
  for (int64_t r = blockIdx.x; r < side; r += gridDim.x) {
    __syncthreads();
    if (int(threadIdx.x) < d) {
      ur[threadIdx.x] = U[int64_t(threadIdx.x) * side + r];
      qr[threadIdx.x] = nside ? Qn[int64_t(threadIdx.x) * side + r] : 0.0;
    }
    __syncthreads();
    for (int64_t c = threadIdx.x; c < side; c += 256) {
      double corr = 0.0;
      if (nside)
        for (int a = 0; a < d; ++a) corr += qr[a] * U[int64_t(a) * side + c] + ur[a] * Qn[int64_t(a) * side + c];
      else
        for (int a = 0; a < d; ++a) corr += ur[a] * U[int64_t(a) * side + c];
      const double v = G[r * side + c] - corr;
      acc += v * v;
    }
  }
  acc = block_sum<4>(acc, sh);
  if (threadIdx.x == 0) gpart[blockIdx.x] = acc;
}

// L_i = sqrt(the partials summed in workgroup order) / n + mu (cca_zoo/linear/_iterative.py:481)
__global__ void __launch_bounds__(256) k_als_admm_lfinal(const double* __restrict__ gpart, int ng, int n, double mu,
                                                        double* __restrict__ lip, const AlsStatus* st) {
  if (admm_not_first(st)) return;
  __shared__ double sh[4];
  const double s = block_sum<4>(int(threadIdx.x) < ng ? gpart[threadIdx.x] : 0.0, sh);
  if (threadIdx.x == 0) *lip = sqrt(s) / double(n) + mu;
}

// The Gram of the centred view on one side, fp64 on v_mfma_f64_16x16x4f64 (lane maps as in kernel_matrix.hip: A operand
// m = lane & 15, k = lane >> 4; B operand k = lane >> 4, n = lane & 15; C/D col = lane & 15, row = (lane >> 4) + 4 reg).
// NSIDE: G[i][j] = sum_f x(i, f) x(j, f) over the p features (i, j rows); else G[i][j] = sum_r x(r, i) x(r, j) over the n
// rows (i, j features); x = fl(X - mu) in the views' precision, as k_als_score rounds it.  256 threads, a 64 x 64 tile per
// workgroup, each wave a 32 x 32 quarter; only tiles on and above the diagonal run, mirror_upper copies them down.
template <typename T, bool NSIDE>
__device__ __forceinline__ void gram_stage(const T* __restrict__ X, const T* __restrict__ mu, int64_t ld, int64_t side, int64_t klen,
                                           int64_t i0, int64_t k0, double* lds) {
#pragma unroll
  for (int e = 0; e < ALS_GT * ALS_GKC / 256; ++e) {
    const int idx = threadIdx.x + 256 * e;
    // consecutive threads read consecutive addresses: features along a row
    const int row = NSIDE ? idx / ALS_GKC : idx % ALS_GT, kk = NSIDE ? idx % ALS_GKC : idx / ALS_GT;
    const int64_t i = i0 + row, kg = k0 + kk;
    double v = 0.0;
    if (i < side && kg < klen) {
      const int64_t r = NSIDE ? i : kg, f = NSIDE ? kg : i;
      const T x = X[r * ld + f];
      v = double(mu ? T(x - mu[f]) : x);
    }
    lds[row * ALS_GLD + kk] = v;
  }
}

template <typename T, bool NSIDE>
__global__ void __launch_bounds__(256) k_als_gram(const T* __restrict__ X, const T* __restrict__ mu, int64_t ld, int64_t side,
                                                 int64_t klen, double* __restrict__ G) {
  if (blockIdx.x < blockIdx.y) return;   // strictly below the diagonal: mirrored afterwards
  typedef double v4f64 __attribute__((ext_vector_type(4)));
  __shared__ double As[ALS_GT * ALS_GLD];
  __shared__ double Bs[ALS_GT * ALS_GLD];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int lr = lane & 15, lk = lane >> 4;
  const int wr = w >> 1, wc = w & 1;
  const int64_t i0 = int64_t(blockIdx.y) * ALS_GT, j0 = int64_t(blockIdx.x) * ALS_GT;
  v4f64 acc[2][2];
#pragma unroll
  for (int a = 0; a < 2; ++a)
#pragma unroll
    for (int b = 0; b < 2; ++b) acc[a][b] = v4f64{0.0, 0.0, 0.0, 0.0};
  for (int64_t k0 = 0; k0 < klen; k0 += ALS_GKC) {
    gram_stage<T, NSIDE>(X, mu, ld, side, klen, i0, k0, As);
    gram_stage<T, NSIDE>(X, mu, ld, side, klen, j0, k0, Bs);
    __syncthreads();
#pragma unroll
    for (int kk = 0; kk < ALS_GKC; kk += 4) {
      double a[2], b[2];
#pragma unroll
      for (int t = 0; t < 2; ++t) {
        a[t] = As[(32 * wr + 16 * t + lr) * ALS_GLD + kk + lk];
        b[t] = Bs[(32 * wc + 16 * t + lr) * ALS_GLD + kk + lk];
      }
#pragma unroll
      for (int ta = 0; ta < 2; ++ta)
#pragma unroll
        for (int tb = 0; tb < 2; ++tb) acc[ta][tb] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[ta], b[tb], acc[ta][tb], 0, 0, 0);
    }
    __syncthreads();
  }
#pragma unroll
  for (int tb = 0; tb < 2; ++tb) {
    const int64_t j = j0 + 32 * wc + 16 * tb + lr;
    if (j >= side) continue;
#pragma unroll
    for (int ta = 0; ta < 2; ++ta)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int64_t i = i0 + 32 * wr + 16 * ta + lk + 4 * r;
        if (i < side) G[i * side + j] = acc[ta][tb][r];
      }
  }
}

// ---- SCCA_IPLS / ElasticCCA: the elastic-net solve in Gram form -------------------------------------------------------------
// argmin_c 1/2 |X_d c - t|^2 + a |c|_1 + b/2 |c|^2 (a = n alpha l1, b = n alpha (1 - l1); the reference's Ridge: a = 0,
// b = alpha) from G = X_d' X_d, q = X_d' t and t't alone.  r = q - G c is carried along.
__device__ __forceinline__ bool enet_off(const AlsStatus* st, int view, int phase) {
  return fit_stopped(st) || st->view != view || st->phase != phase;
}

// t of view i (every view's score when all != 0, cca_zoo/linear/_iterative.py:824-828), t't into scal[0], t~ into B.tt
__global__ void __launch_bounds__(ALS_PT) k_als_enet_prologue(AlsBuf B, AlsViews vw, int i, int all, const AlsStatus* st) {
  if (enet_off(st, i, 0)) return;
  __shared__ double sh[ALS_PT / 64];
  __shared__ double coef[ALS_MAXK];
  const int d = st->dim;
  als_target(B, vw, all ? -1 : i, d, coef, sh);
  double acc = 0.0;
  for (int r = threadIdx.x; r < B.n; r += ALS_PT) acc += B.tt[r] * B.tt[r];      // own rows
  const double tn = block_sum<ALS_PT / 64>(acc, sh);
  if (threadIdx.x == 0) B.scal[4 * i] = tn;
  als_correct_target(B, i, d, coef, sh);
}

// q = the chunk partials of X' t~ summed in chunk order, into raw; r = q - G c with c the view's previous coefficients, or
// c = 0 and r = q at the first solve of a dimension (the reference builds fresh regressors per dimension).  One wave per row.
__global__ void __launch_bounds__(256) k_als_enet_rinit(const double* __restrict__ xpart, int nchunk, int64_t p,
                                                       const double* __restrict__ G, double* __restrict__ c,
                                                       double* __restrict__ raw, double* __restrict__ res, int view,
                                                       const AlsStatus* st) {
  if (enet_off(st, view, 0)) return;
  const int64_t row = int64_t(blockIdx.x) * 4 + (threadIdx.x >> 6);
  if (row >= p) return;
  const int lane = threadIdx.x & 63;
  double q = 0.0;
  for (int ch = 0; ch < nchunk; ++ch) q += xpart[int64_t(ch) * p + row];
  if (st->sweep == 0) {                  // no thread reads c in this branch
    if (lane == 0) { raw[row] = q; res[row] = q; c[row] = 0.0; }
    return;
  }
  double s = 0.0;
  for (int64_t f = lane; f < p; f += 64) s += G[row * p + f] * c[f];
  s = wave_sum(s);
  if (lane == 0) { raw[row] = q; res[row] = q - s; }
}

// (view, phase) -> (to_view, to_phase), one thread; a solve starts with its sweep count at zero
__global__ void k_als_enet_step(AlsStatus* st, int view, int phase, int to_view, int to_phase) {
  if (enet_off(st, view, phase)) return;
  st->view = to_view;
  st->phase = to_phase;
  if (to_phase == 1) st->isweep = 0;
}

// The ENET_BW sequential coordinate steps of block `blk`, one wave: lane l owns coordinate j0 + l, the diagonal tile of G
// lies in LDS by rows (G is symmetric: row j is column j, read without bank conflicts).  Step j:
//   z = r_j + G_jj c_j;  c_j' = sign(z) max(|z| - a, 0) / (G_jj + b);  r -= (c_j' - c_j) G[:, j]  on the block's slice of r
// (G_jj = 0: the coordinate is skipped, as scikit-learn skips zero columns).  The block's changes go to dl for
// k_als_enet_update, max |delta| and max |c| to bstat.
__global__ void __launch_bounds__(ENET_BW) k_als_enet_block(const double* __restrict__ G, int64_t p, double* __restrict__ res,
                                                           double* __restrict__ c, double a, double b, int blk,
                                                           double* __restrict__ dl, double* __restrict__ bstat, int view,
                                                           const AlsStatus* st) {
  if (enet_off(st, view, 1)) return;
  __shared__ double T[ENET_BW * ENET_BW];
  const int lane = threadIdx.x;
  const int64_t j0 = int64_t(blk) * ENET_BW;
  const int bw = int(min(int64_t(ENET_BW), p - j0));
  const bool live = lane < bw;
  for (int j = 0; j < ENET_BW; ++j) T[j * ENET_BW + lane] = (j < bw && live) ? G[(j0 + j) * p + j0 + lane] : 0.0;
  __syncthreads();
  double rl = live ? res[j0 + lane] : 0.0, cl = live ? c[j0 + lane] : 0.0, dmine = 0.0;
  const double g = T[lane * ENET_BW + lane];
  for (int j = 0; j < bw; ++j) {
    const double z = rl + g * cl;
    const double nw = g == 0.0 ? cl : als_soft(z, a) / (g + b);
    const double d = __shfl(nw - cl, j, 64);
    if (lane == j) { cl = nw; dmine = d; }
    if (d != 0.0) rl -= d * T[j * ENET_BW + lane];      // uniform over the wave
  }
  if (live) { res[j0 + lane] = rl; c[j0 + lane] = cl; }
  dl[lane] = dmine;
  const double dmax = wave_max(fabs(dmine)), cmax = wave_max(fabs(cl));
  if (lane == 0) { bstat[2 * blk] = dmax; bstat[2 * blk + 1] = cmax; }
}

// r_f -= sum_j delta_j G[j0 + j][f] for every f outside the block, j in order (the same sums as one coordinate at a time);
// returns at once when the block changed nothing.  One thread per f, 64 per workgroup: p / 64 workgroups fill the device
// at the widths where this kernel's time matters.
__global__ void __launch_bounds__(ENET_BW) k_als_enet_update(const double* __restrict__ G, int64_t p, double* __restrict__ res,
                                                            const double* __restrict__ dl, const double* __restrict__ bstat,
                                                            int blk, int view, const AlsStatus* st) {
  if (enet_off(st, view, 1)) return;
  if (bstat[2 * blk] == 0.0) return;
  __shared__ double dsh[ENET_BW];
  dsh[threadIdx.x] = dl[threadIdx.x];
  __syncthreads();
  const int64_t j0 = int64_t(blk) * ENET_BW, f = int64_t(blockIdx.x) * ENET_BW + threadIdx.x;
  const int bw = int(min(int64_t(ENET_BW), p - j0));
  if (f >= p || (f >= j0 && f < j0 + ENET_BW)) return;
  double acc = res[f];
  for (int j = 0; j < bw; ++j) {
    const double d = dsh[j];
    if (d != 0.0) acc -= d * G[(j0 + j) * p + f];
  }
  res[f] = acc;
}

// After a CD sweep: scikit-learn's stop rule.  With max |delta| / max |c| < tol (or max |c| = 0, or at the cap) the duality
// gap from R'R = t't - c'q - c'r, R't = t't - c'q, X'R = r; the solve ends (phase 2) when gap < tol t't or at the cap.
// ridge: ends on the coordinate change alone.
__global__ void __launch_bounds__(ALS_PT) k_als_enet_check(int64_t p, const double* __restrict__ q, const double* __restrict__ res,
                                                          const double* __restrict__ c, const double* __restrict__ bstat, int nb,
                                                          double a, double b, int ridge, double tol, double* __restrict__ scal,
                                                          int view, AlsStatus* st) {
  if (enet_off(st, view, 1)) return;
  __shared__ double sh[ALS_PT / 64];
  const int t = threadIdx.x;
  const double dmax = block_max<ALS_PT / 64>(t < nb ? bstat[2 * t] : 0.0, sh);
  const double cmax = block_max<ALS_PT / 64>(t < nb ? bstat[2 * t + 1] : 0.0, sh);
  const int isweep = st->isweep + 1;
  const bool crit = cmax == 0.0 || dmax / cmax < tol, cap = isweep >= ENET_CAP;
  bool done = ridge ? (crit || cap) : false, met = crit;
  double gap = 0.0;
  if (!ridge && (crit || cap)) {         // uniform over the workgroup
    double cq = 0.0, cr = 0.0, l1 = 0.0, cc = 0.0, dual = 0.0;
    for (int64_t f = t; f < p; f += ALS_PT) {
      const double v = c[f], rf = res[f];
      cq += v * q[f];
      cr += v * rf;
      l1 += fabs(v);
      cc += v * v;
      dual = fmax(dual, fabs(rf - b * v));
    }
    cq = block_sum<ALS_PT / 64>(cq, sh);
    cr = block_sum<ALS_PT / 64>(cr, sh);
    l1 = block_sum<ALS_PT / 64>(l1, sh);
    cc = block_sum<ALS_PT / 64>(cc, sh);
    dual = block_max<ALS_PT / 64>(dual, sh);
    const double tn = scal[0], rr = tn - cq - cr, rt = tn - cq;
    double cst = 1.0;
    if (dual > a) {
      cst = a / dual;
      gap = 0.5 * (rr + rr * cst * cst);
    } else {
      gap = rr;
    }
    gap += a * l1 - cst * rt + 0.5 * b * (1.0 + cst * cst) * cc;
    met = gap < tol * tn;
    done = met || cap;
  }
  __syncthreads();                       // every thread has read the status
  if (t == 0) {
    st->isweep = isweep;
    st->inner[st->dim] += 1;
    scal[3] = double(isweep);
    if (!ridge && (crit || cap)) scal[1] = gap;
    if (done) {
      st->phase = 2;
      if (!met) st->capped += 1;
    }
  }
}

// SCCA_IPLS: the population standard deviation of the corrected score of the coefficients (numpy.std: the mean subtracted,
// ddof 0; cca_zoo/linear/_iterative.py:619-622) into scal[2]; when it exceeds 1e-12 the score partials are divided by it,
// so that they are those of w_i = c / std
__global__ void __launch_bounds__(ALS_PT) k_als_enet_std(AlsBuf B, AlsViews vw, int i, const AlsStatus* st) {
  if (enet_off(st, i, 2)) return;
  __shared__ double sh[ALS_PT / 64];
  __shared__ double coef[ALS_MAXK];
  const int n = B.n;
  als_corrected_score(B, vw, i, st->dim, B.tt2, false, coef, sh);
  double acc = 0.0;
  for (int r = threadIdx.x; r < n; r += ALS_PT) acc += B.tt2[r];
  const double mean = block_sum<ALS_PT / 64>(acc, sh) / double(n);
  acc = 0.0;
  for (int r = threadIdx.x; r < n; r += ALS_PT) acc += (B.tt2[r] - mean) * (B.tt2[r] - mean);
  const double sd = sqrt(block_sum<ALS_PT / 64>(acc, sh) / double(n));
  if (threadIdx.x == 0) B.scal[4 * i + 2] = sd;
  if (!(sd > 1e-12)) return;
  double* sp = B.spart + int64_t(i) * B.csmax * n;
  for (int cidx = 0; cidx < vw.cs[i]; ++cidx)
    for (int r = threadIdx.x; r < n; r += ALS_PT) sp[int64_t(cidx) * n + r] /= sd;
}

// w = c (ElasticCCA) or c / std when std > 1e-12 (SCCA_IPLS); per-workgroup partial |w - w_old|^2
__global__ void __launch_bounds__(256) k_als_enet_apply(const double* __restrict__ c, int64_t p, int post, const double* __restrict__ scal,
                                                       double* __restrict__ w, double* __restrict__ dpart, int view,
                                                       const AlsStatus* st) {
  if (enet_off(st, view, 2)) return;
  __shared__ double sh[4];
  const double sd = post ? scal[2] : 1.0;
  const bool divide = post && sd > 1e-12;
  double dd = 0.0;
  for (int64_t f = int64_t(blockIdx.x) * 256 + threadIdx.x; f < p; f += int64_t(gridDim.x) * 256) {
    const double u = divide ? c[f] / sd : c[f];
    const double diff = u - w[f];
    dd += diff * diff;
    w[f] = u;
  }
  dd = block_sum<4>(dd, sh);
  if (threadIdx.x == 0) dpart[blockIdx.x] = dd;
}

// at the end of a dimension: G -= a a' with a the newest column of A = (X - mu)' Q (exact: the Q columns are orthonormal; a
// view that was not deflated has a zero column).  grid (ceil(p / 256), rows strided by gridDim.y)
__global__ void __launch_bounds__(256) k_als_enet_deflate(double* __restrict__ G, int64_t p, const double* __restrict__ A,
                                                         const AlsStatus* st) {
  if (acol_off(st, 1)) return;
  const double* a = A + int64_t(st->dim - 1) * p;
  const int64_t f = int64_t(blockIdx.x) * 256 + threadIdx.x;
  if (f >= p) return;
  const double af = a[f];
  for (int64_t r = blockIdx.y; r < p; r += gridDim.y) G[r * p + f] -= a[r] * af;
}

// ---- column means as the reference forms them ----------------------------------------------------------------------------
// NumPy's v.mean(axis=0) of a row-major array adds the rows in order in the array's own precision and divides by n
// (cca_zoo/_base.py:97-99); one thread per column does exactly that, so the means of device rows equal the reference's bit for bit.
template <typename T>
__global__ void __launch_bounds__(256) k_als_colmeans(const T* __restrict__ X, int64_t ld, int64_t p, int64_t n, T* __restrict__ mean) {
  const int64_t f = int64_t(blockIdx.x) * 256 + threadIdx.x;
  if (f >= p) return;
  T acc = T(0);
#pragma unroll 8
  for (int64_t r = 0; r < n; ++r) acc = acc + X[r * ld + f];
  mean[f] = acc / T(n);
}

// ---- sparse views: CSR for the score pass, CSC for X' t~ and the means -------------------------------------------------
// A sparse view is never densified and never rewritten; centring is implicit, (X - 1 mu') w = X w - (mu' w) 1 and
// (X - 1 mu')' t = X' t - mu (1' t), so no x - mu element is formed and nothing is rounded in the values' precision: a value
// is widened exactly, every product and sum is fp64, and float32 and float64 values holding the same numbers give the same
// bits.  A LINE is a row of the CSR form or a column of the CSC form.  A group of G lanes (a power of two in [4, 64], chosen
// once per view and form from the mean line length: sparse_group) owns a line: lane l takes the entries l, l + G, ... of the
// line in order and the lanes combine by an xor butterfly, so the order of summation depends on the matrix and on G alone.
// The indices are trusted: the caller has checked them (include/ccz.h).
__device__ __forceinline__ double group_sum(double v, int G) {
  for (int o = G >> 1; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// the line a thread works on (-1 past the last), its lane within the group; 256 threads = 256 / G lines per workgroup
__device__ __forceinline__ int64_t sparse_line(int64_t nlines, int G, int* lane) {
  *lane = threadIdx.x & (G - 1);
  const int64_t l = int64_t(blockIdx.x) * (256 / G) + threadIdx.x / G;
  return l < nlines ? l : -1;
}

// sum_e val[e] x[idx[e]] over the entries of line l (0 for l = -1: the lanes still take part in the butterfly)
template <typename V>
__device__ __forceinline__ double sparse_line_dot(const V* __restrict__ val, const int32_t* __restrict__ idx,
                                                  const int64_t* __restrict__ ptr, int64_t l, int lane, int G,
                                                  const double* __restrict__ x) {
  int64_t e0 = 0, e1 = 0;
  if (l >= 0) { e0 = ptr[l]; e1 = ptr[l + 1]; }
  double acc = 0.0;
#pragma unroll 4
  for (int64_t e = e0 + lane; e < e1; e += G) acc += double(val[e]) * x[idx[e]];
  return group_sum(acc, G);
}

// per-workgroup partial sums of sum_f a[f] b[f] (b = NULL: of sum_f a[f]): mu' w for the score, 1' t~ for X' t~.  The readers
// add the partials as als_fold_totals does.  first_only as in k_als_score.
__global__ void __launch_bounds__(256) k_als_sparse_dot(const double* __restrict__ a, const double* __restrict__ b, int64_t len,
                                                       double* __restrict__ part, int first_only, const AlsStatus* st) {
  if (fit_stopped(st)) return;
  if (first_only && (st->sweep != 0 || st->view != 0 || st->phase != 0)) return;
  __shared__ double sh[4];
  double acc = 0.0;
  for (int64_t f = int64_t(blockIdx.x) * 256 + threadIdx.x; f < len; f += int64_t(gridDim.x) * 256) acc += b ? a[f] * b[f] : a[f];
  acc = block_sum<4>(acc, sh);
  if (threadIdx.x == 0) part[blockIdx.x] = acc;
}

// score of a sparse view: spart[r] = sum_e val[e] w[col[e]] - mu' w, an empty row gets -mu' w.  part: the npart partials of
// mu' w (NULL without centring).  Entry conditions as k_als_score.
template <typename V>
__global__ void __launch_bounds__(256) k_als_score_csr(const V* __restrict__ val, const int32_t* __restrict__ col,
                                                      const int64_t* __restrict__ ptr, int n, int G, const double* __restrict__ w,
                                                      const double* __restrict__ part, int npart, double* __restrict__ spart,
                                                      int first_only, const AlsStatus* st) {
  if (fit_stopped(st)) return;
  if (first_only && (st->sweep != 0 || st->view != 0 || st->phase != 0)) return;
  __shared__ double sh[4];
  const double muw = part ? block_sum<4>(int(threadIdx.x) < npart ? part[threadIdx.x] : 0.0, sh) : 0.0;
  int lane;
  const int64_t r = sparse_line(n, G, &lane);
  const double s = sparse_line_dot<V>(val, col, ptr, r, lane, G, w);
  if (r >= 0 && lane == 0) spart[r] = s - muw;
}

// X' t~ of a sparse view: out[f] = sum_e val[e] t~[row[e]] - mu[f] (1' t~), the one chunk k_als_fold then sums.  part: the
// npart partials of 1' t~ (read only when mu is given).
template <typename V>
__global__ void __launch_bounds__(256) k_als_xt_csc(const V* __restrict__ val, const int32_t* __restrict__ row,
                                                   const int64_t* __restrict__ ptr, int64_t p, int G, const double* __restrict__ tt,
                                                   const double* __restrict__ mu, const double* __restrict__ part, int npart,
                                                   double* __restrict__ out, const AlsStatus* st) {
  if (fit_stopped(st)) return;
  __shared__ double sh[4];
  const double tsum = mu ? block_sum<4>(int(threadIdx.x) < npart ? part[threadIdx.x] : 0.0, sh) : 0.0;
  int lane;
  const int64_t f = sparse_line(p, G, &lane);
  const double s = sparse_line_dot<V>(val, row, ptr, f, lane, G, tt);
  if (f >= 0 && lane == 0) out[f] = mu ? s - mu[f] * tsum : s;
}

// float64 column means from the CSC form: the stored entries of a column in the group's order, over n
template <typename V>
__global__ void __launch_bounds__(256) k_sparse_colmeans(const V* __restrict__ val, const int64_t* __restrict__ ptr, int64_t p, int G,
                                                        int64_t n, double* __restrict__ mean) {
  int lane;
  const int64_t f = sparse_line(p, G, &lane);
  int64_t e0 = 0, e1 = 0;
  if (f >= 0) { e0 = ptr[f]; e1 = ptr[f + 1]; }
  double acc = 0.0;
  for (int64_t e = e0 + lane; e < e1; e += G) acc += double(val[e]);
  acc = group_sum(acc, G);
  if (f >= 0 && lane == 0) mean[f] = acc / double(n);
}

// muW[c] = sum_f mu[f] W[f][c]: workgroup c, strided sums and block_sum
__global__ void __launch_bounds__(256) k_sparse_muw(const double* __restrict__ mu, const double* __restrict__ W, int64_t p, int k,
                                                   double* __restrict__ muW) {
  __shared__ double sh[4];
  const int c = blockIdx.x;
  double acc = 0.0;
  for (int64_t f = threadIdx.x; f < p; f += 256) acc += mu[f] * W[f * k + c];
  acc = block_sum<4>(acc, sh);
  if (threadIdx.x == 0) muW[c] = acc;
}

// out (rows x k) = X W - 1 muW' from the CSR form, 8 right-hand sides per pass over a row (muW NULL: no centring)
constexpr int SPARSE_KB = 8;
template <typename V>
__global__ void __launch_bounds__(256) k_sparse_project(const V* __restrict__ val, const int32_t* __restrict__ col,
                                                       const int64_t* __restrict__ ptr, int64_t n, int G, const double* __restrict__ W,
                                                       int k, const double* __restrict__ muW, double* __restrict__ out) {
  int lane;
  const int64_t r = sparse_line(n, G, &lane);
  int64_t e0 = 0, e1 = 0;
  if (r >= 0) { e0 = ptr[r]; e1 = ptr[r + 1]; }
  for (int c0 = 0; c0 < k; c0 += SPARSE_KB) {
    const int kb = min(SPARSE_KB, k - c0);
    double acc[SPARSE_KB];
#pragma unroll
    for (int q = 0; q < SPARSE_KB; ++q) acc[q] = 0.0;
    for (int64_t e = e0 + lane; e < e1; e += G) {
      const double v = double(val[e]);
      const double* wr = W + int64_t(col[e]) * k + c0;
#pragma unroll
      for (int q = 0; q < SPARSE_KB; ++q)
        if (q < kb) acc[q] += v * wr[q];
    }
#pragma unroll
    for (int q = 0; q < SPARSE_KB; ++q) {
      const double s = group_sum(acc[q], G);
      if (r >= 0 && lane == 0 && q < kb) out[r * k + c0 + q] = s - (muW ? muW[c0 + q] : 0.0);
    }
  }
}

// G for lines of nnz / nlines stored entries on average: the smallest power of two that is not below the mean, in [4, 64]
inline int sparse_group(int64_t nnz, int64_t nlines) {
  int g = 4;
  while (g < 64 && int64_t(g) * nlines < nnz) g *= 2;
  return g;
}

inline unsigned sparse_grid(int64_t nlines, int G) { return unsigned((nlines + 256 / G - 1) / (256 / G)); }

// what a call needs of a ccz_sparse_view; the indices themselves are the caller's to check
void check_sparse(const ccz_sparse_view* v, bool csr, bool csc) {
  if (!v) fail(CCZ_EINVAL, "sparse: null view");
  const int64_t lim = int64_t(1) << 31;
  if (v->rows < 1 || v->cols < 1 || v->nnz < 0 || v->rows >= lim || v->cols >= lim || v->nnz >= lim)
    fail(CCZ_EINVAL, "sparse: rows and cols must be in [1, 2^31), nnz in [0, 2^31); got %lld x %lld with %lld entries",
         (long long)v->rows, (long long)v->cols, (long long)v->nnz);
  if (csr && (!v->csr_ptr || (v->nnz > 0 && (!v->csr_val || !v->csr_col)))) fail(CCZ_EINVAL, "sparse: the CSR form is missing");
  if (csc && (!v->csc_ptr || (v->nnz > 0 && (!v->csc_val || !v->csc_row)))) fail(CCZ_EINVAL, "sparse: the CSC form is missing");
}

// ---- host driver ----------------------------------------------------------------------------------------------------
struct AlsState : FitState<AlsStatus> {
  int rule, max_iter;
  int64_t n, k;
  double tol;
  std::vector<double> par;
  AlsBuf B;
  bool has_init = false;
  double mu = 0.0;                 // SCCA_ADMM: the penalty, and what ccz_als_admm_setup left per view
  bool admm_ready = false;
  AdmmView admm[ALS_MAXV] = {};
  int last_cs[ALS_MAXV] = {};
  bool enet_used = false;          // units have run since the setup: G_i is deflated
  bool enet_ready = false;         // elastic net: what ccz_als_enet_setup left per view (admm[i].G = G_i, .U = A_i)
  double ea[ALS_MAXV] = {}, eb[ALS_MAXV] = {};
  int eridge[ALS_MAXV] = {};
  int enet_all = 0, enet_post = 0;
  // sparse views (ccz_als_set_sparse): the two forms, G of the rows and of the columns, the partials of mu' w / 1' t~
  bool sparse[ALS_MAXV] = {};
  bool any_sparse = false;
  ccz_sparse_view sp[ALS_MAXV] = {};
  int grow[ALS_MAXV] = {}, gcol[ALS_MAXV] = {};
  double* sdot = nullptr;          // ALS_MAXG
};

AlsViews make_views(const AlsState& S, const ccz_view* views, const void* const* means) {
  AlsViews vw;
  memset(&vw, 0, sizeof(vw));
  if (S.any_sparse && views) {     // a sparse view's data and ld are ignored, its cols must still match
    ccz_view seen[ALS_MAXV];
    for (int i = 0; i < S.M; ++i) {
      seen[i] = views[i];
      if (S.sparse[i]) { seen[i].data = &S; seen[i].ld = seen[i].cols; }
    }
    fill_views("als", vw, seen, means, S.p);
    for (int i = 0; i < S.M; ++i)
      if (S.sparse[i]) vw.X[i] = nullptr;
  } else {
    fill_views("als", vw, views, means, S.p);
  }
  int64_t off = 0;
  for (int i = 0; i < S.M; ++i) {
    vw.p[i] = S.p[i];
    vw.off[i] = off;
    off += S.p[i];
    vw.cs[i] = S.sparse[i] ? 1 : column_splits(S.n, ALS_SROWS, S.p[i], S.B.csmax);
    vw.ng[i] = int(std::max<int64_t>(1, std::min<int64_t>(ALS_MAXG, (S.p[i] + 2047) / 2048)));
    vw.par[i] = S.par[i];
    vw.rule[i] = (S.rule == RULE_TOP_S && S.par[i] >= double(S.p[i])) ? int(RULE_NORMALISE) : S.rule;
  }
  return vw;
}

// workgroups of k_als_sparse_dot over a vector of len entries (the grids depend on the shapes and on G alone)
inline int sparse_dot_groups(int64_t len) { return int(std::max<int64_t>(1, std::min<int64_t>(ALS_MAXG, (len + 2047) / 2048))); }

// the score of sparse view i: mu' w first (when centring), then the rows
void launch_score_sparse(ccz_ctx* c, const AlsState& S, const AlsViews& vw, int i, int first_only) {
  const ccz_sparse_view& v = S.sp[i];
  const double* w = S.B.w + vw.off[i];
  const double* mu = static_cast<const double*>(vw.mu[i]);
  const int nd = sparse_dot_groups(vw.p[i]);
  if (mu) {
    hipLaunchKernelGGL(k_als_sparse_dot, dim3(nd), dim3(256), 0, stream(c), mu, w, vw.p[i], S.sdot, first_only, S.drv.dev);
    CCZ_LAUNCH_CHECK();
  }
  by_dtype(S.dtype, [&](auto t) {
    using T = decltype(t);
    hipLaunchKernelGGL((k_als_score_csr<T>), dim3(sparse_grid(S.n, S.grow[i])), dim3(256), 0, stream(c),
                       static_cast<const T*>(v.csr_val), v.csr_col, v.csr_ptr, int(S.n), S.grow[i], w, mu ? S.sdot : nullptr, nd,
                       S.B.spart + int64_t(i) * S.B.csmax * S.n, first_only, S.drv.dev);
  });
  CCZ_LAUNCH_CHECK();
}

// X' t~ of sparse view i into the first chunk of xpart: 1' t~ first (when centring), then the columns
void launch_xt_sparse(ccz_ctx* c, const AlsState& S, const AlsViews& vw, int i) {
  const ccz_sparse_view& v = S.sp[i];
  const double* mu = static_cast<const double*>(vw.mu[i]);
  const int nd = sparse_dot_groups(S.n);
  if (mu) {
    hipLaunchKernelGGL(k_als_sparse_dot, dim3(nd), dim3(256), 0, stream(c), S.B.tt, static_cast<const double*>(nullptr), S.n, S.sdot, 0,
                       S.drv.dev);
    CCZ_LAUNCH_CHECK();
  }
  by_dtype(S.dtype, [&](auto t) {
    using T = decltype(t);
    hipLaunchKernelGGL((k_als_xt_csc<T>), dim3(sparse_grid(vw.p[i], S.gcol[i])), dim3(256), 0, stream(c),
                       static_cast<const T*>(v.csc_val), v.csc_row, v.csc_ptr, vw.p[i], S.gcol[i], S.B.tt, mu, S.sdot, nd, S.B.xpart,
                       S.drv.dev);
  });
  CCZ_LAUNCH_CHECK();
}

// vec: the p-vectors scored (B.w unless given); gate: see k_als_score
void launch_score(ccz_ctx* c, const AlsState& S, const AlsViews& vw, int i, int first_only, const double* vec = nullptr, int gate = -1) {
  if (S.sparse[i]) return launch_score_sparse(c, S, vw, i, first_only);     // the plain rules only: no vec, no gate
  const dim3 grid(unsigned((S.n + ALS_SROWS - 1) / ALS_SROWS), unsigned(vw.cs[i]));
  by_dtype(S.dtype, [&](auto t) {
    using T = decltype(t);
    hipLaunchKernelGGL((k_als_score<T>), grid, dim3(256), 0, stream(c), static_cast<const T*>(vw.X[i]), static_cast<const T*>(vw.mu[i]),
                       vw.ld[i], vw.p[i], int(S.n), (vec ? vec : S.B.w) + vw.off[i], S.B.spart + int64_t(i) * S.B.csmax * S.n, first_only,
                       gate, S.drv.dev);
  });
  CCZ_LAUNCH_CHECK();
}

void launch_xt(ccz_ctx* c, const AlsState& S, const AlsViews& vw, int i, int gate = -1) {
  if (S.sparse[i]) return launch_xt_sparse(c, S, vw, i);
  const dim3 grid(unsigned((vw.p[i] + ALS_STRIP - 1) / ALS_STRIP), unsigned(S.B.nchunk));
  by_dtype(S.dtype, [&](auto t) {
    using T = decltype(t);
    hipLaunchKernelGGL((k_als_xt<T>), grid, dim3(256), 0, stream(c), static_cast<const T*>(vw.X[i]), static_cast<const T*>(vw.mu[i]),
                       vw.ld[i], vw.p[i], int(S.n), S.B.rc, S.B.tt, S.B.xpart, gate, S.drv.dev);
  });
  CCZ_LAUNCH_CHECK();
}

// fold .. apply of view i (the rule's passes over raw: 2, or 13 for soft at L1, 16 for top s)
void launch_rule(ccz_ctx* c, const AlsState& S, const AlsViews& vw, int i) {
  const AlsBuf& B = S.B;
  const int rule = vw.rule[i], ng = vw.ng[i];
  const int64_t p = vw.p[i];
  double* raw = B.raw + vw.off[i];
  double* fstat = B.fstat + size_t(i) * ALS_MAXG * 3;
  const int nchunk = S.sparse[i] ? 1 : B.nchunk;     // k_als_xt_csc writes the one chunk
  hipLaunchKernelGGL(k_als_fold, dim3(ng), dim3(256), 0, stream(c), B.xpart, nchunk, p, raw, rule, vw.par[i], fstat, S.drv.dev);
  CCZ_LAUNCH_CHECK();
  if (rule == RULE_SOFT_L1 || rule == RULE_TOP_S) {
    const int passes = rule == RULE_SOFT_L1 ? ALS_PMD_PASSES : ALS_SPAN_PASSES;
    for (int q = 0; q < passes; ++q) {
      hipLaunchKernelGGL(k_als_levels, dim3(ng), dim3(256), 0, stream(c), raw, p, rule, vw.par[i], q, fstat, ng, B.lstate, B.lpart, S.drv.dev);
      CCZ_LAUNCH_CHECK();
    }
    hipLaunchKernelGGL(k_als_norm, dim3(ng), dim3(256), 0, stream(c), raw, p, rule, vw.par[i], passes, fstat, ng, B.lstate, B.lpart,
                       B.thr + 2 * i, B.nstat, S.drv.dev);
    CCZ_LAUNCH_CHECK();
  }
  hipLaunchKernelGGL(k_als_apply, dim3(ng), dim3(256), 0, stream(c), raw, p, rule, vw.par[i], fstat, ng, B.thr + 2 * i, B.nstat, B.w + vw.off[i],
                     B.dpart + size_t(i) * ALS_MAXG, S.drv.dev);
  CCZ_LAUNCH_CHECK();
}

void launch_prologue(ccz_ctx* c, const AlsState& S, const AlsViews& vw, int i) {
  hipLaunchKernelGGL(k_als_prologue, dim3(1), dim3(ALS_PT), 0, stream(c), S.B, vw, i, S.drv.dev);
  CCZ_LAUNCH_CHECK();
}

// p side: the newest column of A_i = (X_i - mu_i)' Q_i (enet: gated on the end of a dimension, else on a dimension's first
// iteration)
void launch_acol(ccz_ctx* c, const AlsState& S, const AlsViews& vw, int i, int enet) {
  const AlsBuf& B = S.B;
  const double* Q = B.Q + int64_t(i) * B.k * S.n;
  const dim3 grid(unsigned((vw.p[i] + 255) / 256), unsigned(B.nchunk));
  by_dtype(S.dtype, [&](auto t) {
    using T = decltype(t);
    hipLaunchKernelGGL((k_als_admm_xtq<T>), grid, dim3(256), 0, stream(c), static_cast<const T*>(vw.X[i]),
                       static_cast<const T*>(vw.mu[i]), vw.ld[i], vw.p[i], int(S.n), B.rc, Q, B.xpart, enet, S.drv.dev);
  });
  CCZ_LAUNCH_CHECK();
  hipLaunchKernelGGL(k_als_admm_afold, dim3(grid.x), dim3(256), 0, stream(c), B.xpart, B.nchunk, vw.p[i], S.admm[i].U, enet, S.drv.dev);
  CCZ_LAUNCH_CHECK();
}

// SCCA_ADMM: L_i at the first iteration of a dimension (the four kernels return at once otherwise)
void launch_admm_lipschitz(ccz_ctx* c, const AlsState& S, const AlsViews& vw, int i) {
  const AlsBuf& B = S.B;
  const AdmmView& a = S.admm[i];
  const double* Q = B.Q + int64_t(i) * B.k * S.n;
  if (S.k > 1 && a.nside) {
    hipLaunchKernelGGL(k_als_admm_kq, dim3(unsigned((S.n + 3) / 4)), dim3(256), 0, stream(c), a.G, int(S.n), Q, a.KQ, S.drv.dev);
    CCZ_LAUNCH_CHECK();
    hipLaunchKernelGGL(k_als_admm_h, dim3(1), dim3(ALS_PT), 0, stream(c), int(S.n), Q, a.KQ, a.U, S.drv.dev);
    CCZ_LAUNCH_CHECK();
  } else if (S.k > 1) {
    launch_acol(c, S, vw, i, 0);
  }
  const int lg = int(std::min<int64_t>(ALS_LG, a.side));
  hipLaunchKernelGGL(k_als_admm_gnorm, dim3(lg), dim3(256), 0, stream(c), a.G, a.side, a.U, Q, a.nside, B.gpart, S.drv.dev);
  CCZ_LAUNCH_CHECK();
  hipLaunchKernelGGL(k_als_admm_lfinal, dim3(1), dim3(256), 0, stream(c), B.gpart, lg, int(S.n), S.mu, B.lip + i, S.drv.dev);
  CCZ_LAUNCH_CHECK();
}

void finish_sweep(ccz_ctx* c, const AlsState& S, const AlsViews& vw) {
  hipLaunchKernelGGL(k_als_finish, dim3(1), dim3(ALS_PT), 0, stream(c), S.B, vw, S.tol, S.max_iter, S.drv.dev);
  CCZ_LAUNCH_CHECK();
  const int ga = int(std::max<int64_t>(1, std::min<int64_t>(256, (S.B.ptot + 2047) / 2048)));
  hipLaunchKernelGGL(k_als_advance, dim3(ga), dim3(256), 0, stream(c), S.B, S.drv.dev);
  CCZ_LAUNCH_CHECK();
}

// one SCCA_ADMM iteration: every view's update reads the scores the iteration started with (Jacobi), so the new vectors are
// scored only after the last update
void enqueue_admm_iteration(ccz_ctx* c, const AlsState& S, const AlsViews& vw) {
  const AlsBuf& B = S.B;
  for (int i = 0; i < S.M; ++i) launch_score(c, S, vw, i, 1);
  for (int i = 0; i < S.M; ++i) {
    launch_admm_lipschitz(c, S, vw, i);
    hipLaunchKernelGGL(k_als_admm_prologue, dim3(1), dim3(ALS_PT), 0, stream(c), B, vw, i, S.drv.dev);
    CCZ_LAUNCH_CHECK();
    launch_xt(c, S, vw, i);
    const int ng = vw.ng[i];
    const double thr = vw.par[i] / S.mu;
    double* fstat = B.fstat + size_t(i) * ALS_MAXG * 3;
    hipLaunchKernelGGL(k_als_admm_fold, dim3(ng), dim3(256), 0, stream(c), B.xpart, B.nchunk, vw.p[i], B.w + vw.off[i], B.eta + vw.off[i],
                       B.lip + i, S.mu, thr, B.raw + vw.off[i], fstat, S.drv.dev);
    CCZ_LAUNCH_CHECK();
    hipLaunchKernelGGL(k_als_admm_apply, dim3(ng), dim3(256), 0, stream(c), B.raw + vw.off[i], vw.p[i], thr, fstat, ng, B.w + vw.off[i],
                       B.eta + vw.off[i], B.dpart + size_t(i) * ALS_MAXG, S.drv.dev);
    CCZ_LAUNCH_CHECK();
  }
  for (int i = 0; i < S.M; ++i) launch_score(c, S, vw, i, 0);
  finish_sweep(c, S, vw);
}

// elastic net: `sweeps` CD sweeps of view i's running solve (every kernel passes unless the status says view i, phase 1)
void enqueue_cd(ccz_ctx* c, const AlsState& S, const AlsViews& vw, int i, int64_t sweeps) {
  const AlsBuf& B = S.B;
  const int64_t p = vw.p[i];
  const int nb = int((p + ENET_BW - 1) / ENET_BW);
  const double* G = S.admm[i].G;
  double* coef = B.coef + vw.off[i];
  for (int64_t s = 0; s < sweeps; ++s) {
    for (int b = 0; b < nb; ++b) {
      hipLaunchKernelGGL(k_als_enet_block, dim3(1), dim3(ENET_BW), 0, stream(c), G, p, B.res, coef, S.ea[i], S.eb[i], b, B.dl, B.bstat, i,
                         S.drv.dev);
      CCZ_LAUNCH_CHECK();
      if (nb == 1) continue;             // no r outside the block
      hipLaunchKernelGGL(k_als_enet_update, dim3(nb), dim3(ENET_BW), 0, stream(c), G, p, B.res, B.dl, B.bstat, b, i, S.drv.dev);
      CCZ_LAUNCH_CHECK();
    }
    hipLaunchKernelGGL(k_als_enet_check, dim3(1), dim3(ALS_PT), 0, stream(c), p, B.raw + vw.off[i], B.res, coef, B.bstat, nb, S.ea[i], S.eb[i],
                       S.eridge[i], S.tol, B.scal + 4 * i, i, S.drv.dev);
    CCZ_LAUNCH_CHECK();
  }
}

void launch_enet_step(ccz_ctx* c, const AlsState& S, int view, int phase, int to_view, int to_phase) {
  hipLaunchKernelGGL(k_als_enet_step, dim3(1), dim3(1), 0, stream(c), S.drv.dev, view, phase, to_view, to_phase);
  CCZ_LAUNCH_CHECK();
}

// r = q - G c of view i from the chunk partials in xpart, then phase 1
void launch_enet_rinit(ccz_ctx* c, const AlsState& S, const AlsViews& vw, int i) {
  const AlsBuf& B = S.B;
  hipLaunchKernelGGL(k_als_enet_rinit, dim3(unsigned((vw.p[i] + 3) / 4)), dim3(256), 0, stream(c), B.xpart, B.nchunk, vw.p[i], S.admm[i].G,
                     B.coef + vw.off[i], B.raw + vw.off[i], B.res, i, S.drv.dev);
  CCZ_LAUNCH_CHECK();
  launch_enet_step(c, S, i, 0, i, 1);
}

// one unit of an elastic-net fit (see the head of the file)
void enqueue_enet_unit(ccz_ctx* c, const AlsState& S, const AlsViews& vw) {
  const AlsBuf& B = S.B;
  for (int i = 0; i < S.M; ++i) launch_score(c, S, vw, i, 1);
  for (int i = 0; i < S.M; ++i) {
    hipLaunchKernelGGL(k_als_enet_prologue, dim3(1), dim3(ALS_PT), 0, stream(c), B, vw, i, S.enet_all, S.drv.dev);
    CCZ_LAUNCH_CHECK();
    launch_xt(c, S, vw, i, i);
    launch_enet_rinit(c, S, vw, i);
    const int64_t nb = (vw.p[i] + ENET_BW - 1) / ENET_BW;
    enqueue_cd(c, S, vw, i, std::max<int64_t>(1, std::min<int64_t>(ENET_CD_CHUNK, ENET_CD_BLOCKS / nb)));
    launch_score(c, S, vw, i, 0, B.coef, i);
    if (S.enet_post) {
      hipLaunchKernelGGL(k_als_enet_std, dim3(1), dim3(ALS_PT), 0, stream(c), B, vw, i, S.drv.dev);
      CCZ_LAUNCH_CHECK();
    }
    hipLaunchKernelGGL(k_als_enet_apply, dim3(vw.ng[i]), dim3(256), 0, stream(c), B.coef + vw.off[i], vw.p[i], S.enet_post, B.scal + 4 * i,
                       B.w + vw.off[i], B.dpart + size_t(i) * ALS_MAXG, i, S.drv.dev);
    CCZ_LAUNCH_CHECK();
    launch_enet_step(c, S, i, 2, i + 1, 0);
  }
  finish_sweep(c, S, vw);
  if (S.k == 1) return;
  for (int i = 0; i < S.M; ++i) {
    launch_acol(c, S, vw, i, 1);
    const int64_t p = vw.p[i];
    hipLaunchKernelGGL(k_als_enet_deflate, dim3(unsigned((p + 255) / 256), unsigned(std::min<int64_t>(p, 256))), dim3(256), 0, stream(c),
                       S.admm[i].G, p, S.admm[i].U, S.drv.dev);
    CCZ_LAUNCH_CHECK();
  }
}

void enqueue_sweep(ccz_ctx* c, const AlsState& S, const AlsViews& vw) {
  if (S.rule == RULE_ADMM) return enqueue_admm_iteration(c, S, vw);
  if (S.rule == RULE_ENET) return enqueue_enet_unit(c, S, vw);
  for (int i = 0; i < S.M; ++i) launch_score(c, S, vw, i, 1);
  for (int i = 0; i < S.M; ++i) {
    launch_prologue(c, S, vw, i);
    launch_xt(c, S, vw, i);
    launch_rule(c, S, vw, i);
    launch_score(c, S, vw, i, 0);
  }
  finish_sweep(c, S, vw);
}

AlsState* als_create(ccz_ctx* c, int dtype, int M, const int64_t* p, int64_t n, int64_t k, int rule, const double* par, double tol,
                     int64_t max_iter, int64_t chunk) {
  check_dtype("als", dtype);
  check_view_count("als", M, ALS_MAXV);
  if (k < 1 || k > ALS_MAXK) fail(CCZ_EUNSUP, "als: 1 to %d latent dimensions are supported, got %lld", ALS_MAXK, (long long)k);
  if (!p || n < 1 || n > (int64_t(1) << 30) || max_iter < 1 || max_iter > (int64_t(1) << 30) || chunk < 1 || !(tol >= 0.0))
    fail(CCZ_EINVAL, "als: bad argument");
  if (rule < RULE_NORMALISE || rule > RULE_ENET) fail(CCZ_EINVAL, "als: unknown rule %d", rule);
  if (rule != RULE_NORMALISE && !par) fail(CCZ_EINVAL, "als: the rule needs one parameter per view");
  check_no_empty_view("als", M, p);
  return new_state<AlsState>(c, [&](AlsState& S) {
    S.dtype = dtype; S.M = M; S.rule = rule; S.max_iter = int(max_iter);
    S.n = n; S.k = k; S.chunk = chunk; S.tol = tol;
    AlsBuf& B = S.B;
    memset(&B, 0, sizeof(B));
    B.n = int(n); B.M = M; B.k = int(k);
    for (int i = 0; i < M; ++i) {
      if (rule == RULE_ADMM && std::min(n, p[i]) > ALS_ADMM_MAXSIDE)
        fail(CCZ_EUNSUP, "als: ADMM keeps a min(n, p) x min(n, p) Gram per view; view %d has min(n, p) = %lld > %d", i,
             (long long)std::min(n, p[i]), ALS_ADMM_MAXSIDE);
      if (rule == RULE_ENET && p[i] > ENET_MAXP)
        fail(CCZ_EUNSUP, "als: the elastic-net models keep a p x p Gram per view; view %d has p = %lld > %d", i, (long long)p[i], ENET_MAXP);
      const double q = par ? par[i] : 0.0;
      if (rule == RULE_TOP_S && !(q >= 1.0)) fail(CCZ_EINVAL, "als: top-s needs s >= 1 (view %d)", i);
      if (rule != RULE_NORMALISE && !(q == q)) fail(CCZ_EINVAL, "als: the parameter of view %d is NaN", i);
      S.p.push_back(p[i]);
      S.par.push_back(q);
      B.ptot += p[i];
      B.pmax = std::max(B.pmax, p[i]);
    }
    B.csmax = 16;
    row_chunks(n, 64, &B.nchunk, &B.rc);
    B.w = S.get(c, size_t(B.ptot));
    B.raw = S.get(c, size_t(B.ptot));
    B.init = S.get(c, size_t(B.ptot) * k);
    B.Wout = S.get(c, size_t(B.ptot) * k);
    B.spart = S.get(c, size_t(M) * B.csmax * n);
    B.Q = S.get(c, size_t(M) * k * n);
    B.tt = S.get(c, size_t(n));
    B.xpart = S.get(c, size_t(B.nchunk) * B.pmax);
    B.fstat = S.get(c, size_t(M) * ALS_MAXG * 3);
    B.lpart = S.get(c, size_t(2) * ALS_MAXG * ALS_NC);
    B.lstate = S.get(c, size_t(2) * (ALS_SPAN_PASSES + 1));
    B.nstat = S.get(c, ALS_MAXG);
    B.thr = S.get(c, size_t(M) * 2);
    B.dpart = S.get(c, size_t(M) * ALS_MAXG);
    S.sdot = S.get(c, ALS_MAXG);
    if (rule == RULE_ADMM) {
      B.eta = S.get(c, size_t(B.ptot));
      B.tt2 = S.get(c, size_t(n));
      B.lip = S.get(c, size_t(M));
      B.gpart = S.get(c, ALS_LG);
      for (int i = 0; i < M; ++i) {
        AdmmView& a = S.admm[i];
        a.nside = n <= p[i] ? 1 : 0;
        a.side = std::min(n, p[i]);
        a.G = S.get(c, size_t(a.side) * a.side);
        a.U = S.get(c, size_t(k) * a.side);
        a.KQ = a.nside ? S.get(c, size_t(k) * n) : nullptr;
      }
    }
    if (rule == RULE_ENET) {
      B.enet = 1;
      B.tt2 = S.get(c, size_t(n));
      B.coef = S.get(c, size_t(B.ptot));
      B.res = S.get(c, size_t(B.pmax));
      B.dl = S.get(c, ENET_BW);
      B.bstat = S.get(c, size_t(2) * ((B.pmax + ENET_BW - 1) / ENET_BW));
      B.scal = S.get(c, size_t(M) * 4);
      for (int i = 0; i < M; ++i) {
        AdmmView& a = S.admm[i];
        a.nside = 0;                       // on the p side whatever n is
        a.side = p[i];
        a.G = S.get(c, size_t(p[i]) * p[i]);
        a.U = S.get(c, size_t(k) * p[i]);
        a.KQ = nullptr;
      }
    }
    S.drv.create(c);
  });
}

// SCCA_ADMM: the penalty and the Gram of every centred view on its smaller side
template <typename T>
void launch_gram(ccz_ctx* c, const AlsState& S, const AlsViews& vw, int i) {
  const AdmmView& a = S.admm[i];
  const unsigned nb = unsigned((a.side + ALS_GT - 1) / ALS_GT);
  const T* X = static_cast<const T*>(vw.X[i]);
  const T* mu = static_cast<const T*>(vw.mu[i]);
  if (a.nside)
    hipLaunchKernelGGL((k_als_gram<T, true>), dim3(nb, nb), dim3(256), 0, stream(c), X, mu, vw.ld[i], a.side, vw.p[i], a.G);
  else
    hipLaunchKernelGGL((k_als_gram<T, false>), dim3(nb, nb), dim3(256), 0, stream(c), X, mu, vw.ld[i], a.side, S.n, a.G);
  CCZ_LAUNCH_CHECK();
  mirror_upper(c, a.side, a.G, a.side);
}

void als_admm_setup(ccz_ctx* c, AlsState& S, const ccz_view* views, const void* const* means, double mu) {
  if (S.rule != RULE_ADMM) fail(CCZ_EINVAL, "als: the fit state was not created with CCZ_ALS_ADMM");
  if (!(mu > 0.0) || !std::isfinite(mu)) fail(CCZ_EINVAL, "als: mu must be positive and finite");
  const AlsViews vw = make_views(S, views, means);
  for (int i = 0; i < S.M; ++i) by_dtype(S.dtype, [&](auto t) { launch_gram<decltype(t)>(c, S, vw, i); });
  S.mu = mu;
  S.admm_ready = true;
}

// SCCA_IPLS / ElasticCCA: the penalties, the two outer rules, and G_i = fl(X_i - mu_i)' fl(X_i - mu_i) of every view.  The fit
// deflates G_i in place, so every fit needs a setup of its own.
void als_enet_setup(ccz_ctx* c, AlsState& S, const ccz_view* views, const void* const* means, const double* a, const double* b,
                    const int* ridge, int target_all, int post_std) {
  if (S.rule != RULE_ENET) fail(CCZ_EINVAL, "als: the fit state was not created with CCZ_ALS_ENET");
  if (!a || !b || !ridge) fail(CCZ_EINVAL, "als: null argument");
  for (int i = 0; i < S.M; ++i) {
    if (!(a[i] >= 0.0) || !(b[i] >= 0.0) || !std::isfinite(a[i]) || !std::isfinite(b[i]))
      fail(CCZ_EINVAL, "als: the penalties of view %d must be finite and not negative", i);
    if (ridge[i] && a[i] != 0.0) fail(CCZ_EINVAL, "als: the ridge solve of view %d takes no L1 penalty", i);
    S.ea[i] = a[i]; S.eb[i] = b[i]; S.eridge[i] = ridge[i] ? 1 : 0;
  }
  S.enet_all = target_all ? 1 : 0;
  S.enet_post = post_std ? 1 : 0;
  const AlsViews vw = make_views(S, views, means);
  for (int i = 0; i < S.M; ++i) by_dtype(S.dtype, [&](auto t) { launch_gram<decltype(t)>(c, S, vw, i); });
  zero(c, S.B.coef, size_t(S.B.ptot) * 8);
  zero(c, S.B.scal, size_t(S.M) * 32);
  S.enet_ready = true;
  S.enet_used = false;
}

// One solve of view `view` outside a fit (what the kernel tests drive): G (p x p, null keeps the view's own), q and the
// starting coefficients from the host, t't = tt; r = q - G c, then n_sweeps CD sweeps under the stop rule.  The status is
// left at (view, phase 1 or 2), so a fit must begin with ccz_als_set_init.
void als_enet_solve(ccz_ctx* c, AlsState& S, int view, const double* G, const double* q, const double* c0, double tt, int64_t n_sweeps) {
  const AlsBuf& B = S.B;
  AlsViews vw;
  memset(&vw, 0, sizeof(vw));
  int64_t off = 0;
  for (int i = 0; i < S.M; ++i) { vw.p[i] = S.p[i]; vw.off[i] = off; off += S.p[i]; }
  const int64_t p = S.p[view];
  sync(c);
  if (G) h2d(c, S.admm[view].G, G, size_t(p) * p * 8);
  h2d(c, B.coef + vw.off[view], c0, size_t(p) * 8);
  // q as the single chunk partial of k_als_enet_rinit
  h2d(c, B.xpart, q, size_t(p) * 8);
  h2d(c, B.scal + 4 * view, &tt, 8);
  AlsStatus st0;
  memset(&st0, 0, sizeof(st0));
  st0.view = view;
  st0.sweep = 1;                         // not a dimension's first solve: start from c0
  h2d(c, S.drv.dev, &st0, sizeof(st0));
  hipLaunchKernelGGL(k_als_enet_rinit, dim3(unsigned((p + 3) / 4)), dim3(256), 0, stream(c), B.xpart, 1, p, S.admm[view].G,
                     B.coef + vw.off[view], B.raw + vw.off[view], B.res, view, S.drv.dev);
  CCZ_LAUNCH_CHECK();
  launch_enet_step(c, S, view, 0, view, 1);
  enqueue_cd(c, S, vw, view, n_sweeps);
  S.has_init = false;
  S.enet_used = true;
}

void als_set_init(ccz_ctx* c, AlsState& S, const double* w0) {
  if (!w0) fail(CCZ_EINVAL, "als: null initial vectors");
  const AlsBuf& B = S.B;
  h2d(c, B.init, w0, size_t(B.ptot) * S.k * 8);
  h2d(c, B.w, w0, size_t(B.ptot) * 8);
  zero(c, B.Wout, size_t(B.ptot) * S.k * 8);
  zero(c, B.Q, size_t(S.M) * S.k * S.n * 8);
  zero(c, B.thr, size_t(S.M) * 16);
  if (S.rule == RULE_ENET && S.enet_used) fail(CCZ_EINVAL, "als: ccz_als_enet_setup must precede every elastic-net fit (the last one deflated G)");
  AlsStatus st0;
  memset(&st0, 0, sizeof(st0));
  h2d(c, S.drv.dev, &st0, sizeof(st0));
  S.has_init = true;
}

}  // namespace
}  // namespace ccz

extern "C" {

int ccz_als_create(ccz_handle h, int dtype, int n_views, const int64_t* p, int64_t n_rows, int64_t k, int rule,
                   const double* rule_param, double tol, int64_t max_iter, int64_t chunk_sweeps, void** state_out) {
  CCZ_GUARD(h, {
    if (!state_out) ccz::fail(CCZ_EINVAL, "null argument");
    *state_out = nullptr;
    *state_out = ccz::als_create(h, dtype, n_views, p, n_rows, k, rule, rule_param, tol, max_iter, chunk_sweeps);
  })
}

int ccz_als_destroy(ccz_handle h, void* state) {
  CCZ_GUARD(h, {
    if (state) ccz::free_state(h, static_cast<ccz::AlsState*>(state));
  })
}

int ccz_als_set_init(ccz_handle h, void* state, const double* w0_host) {
  CCZ_GUARD(h, {
    ccz::AlsState& S = *ccz::as_state<ccz::AlsState>("als", state);
    S.restart(h);
    ccz::als_set_init(h, S, w0_host);
  })
}

int ccz_als_admm_setup(ccz_handle h, void* state, const ccz_view* views, const void* const* means_dev, double mu) {
  CCZ_GUARD(h, {
    ccz::AlsState& S = *ccz::as_state<ccz::AlsState>("als", state);
    ccz::als_admm_setup(h, S, views, means_dev, mu);
  })
}

int ccz_als_enet_setup(ccz_handle h, void* state, const ccz_view* views, const void* const* means_dev, const double* a,
                       const double* b, const int* ridge, int target_all, int post_std) {
  CCZ_GUARD(h, {
    ccz::AlsState& S = *ccz::as_state<ccz::AlsState>("als", state);
    ccz::als_enet_setup(h, S, views, means_dev, a, b, ridge, target_all, post_std);
  })
}

int ccz_als_enet_solve(ccz_handle h, void* state, int view, const double* G_host, const double* q_host, const double* c0_host,
                       double tt, int64_t n_sweeps) {
  CCZ_GUARD(h, {
    ccz::AlsState& S = *ccz::as_state<ccz::AlsState>("als", state);
    if (S.rule != ccz::RULE_ENET || !S.enet_ready) ccz::fail(CCZ_EINVAL, "als: ccz_als_enet_setup has not been called");
    if (view < 0 || view >= S.M || !q_host || !c0_host || n_sweeps < 0 || n_sweeps > ccz::ENET_CAP) ccz::fail(CCZ_EINVAL, "als: bad argument");
    ccz::als_enet_solve(h, S, view, G_host, q_host, c0_host, tt, n_sweeps);
  })
}

int ccz_als_enet_status(ccz_handle h, void* state, int64_t* cd_sweeps_per_dim, int64_t* capped) {
  CCZ_GUARD(h, {
    ccz::AlsState& S = *ccz::as_state<ccz::AlsState>("als", state);
    ccz::AlsStatus st;
    ccz::d2h(h, &st, S.drv.dev, sizeof(st));
    for (int64_t d = 0; d < S.k; ++d)
      if (cd_sweeps_per_dim) cd_sweeps_per_dim[d] = st.inner[d];
    if (capped) *capped = st.capped;
  })
}

int ccz_als_sweeps(ccz_handle h, void* state, const ccz_view* views, const void* const* means_dev, int64_t n_sweeps,
                   int64_t* sweeps_known, int* stopped_known) {
  CCZ_GUARD(h, {
    ccz::AlsState& S = *ccz::as_state<ccz::AlsState>("als", state);
    if (!S.has_init) ccz::fail(CCZ_EINVAL, "als: ccz_als_set_init has not been called");
    if (S.rule == ccz::RULE_ADMM && !S.admm_ready) ccz::fail(CCZ_EINVAL, "als: ccz_als_admm_setup has not been called");
    if (S.rule == ccz::RULE_ENET) {
      if (!S.enet_ready) ccz::fail(CCZ_EINVAL, "als: ccz_als_enet_setup has not been called");
      S.enet_used = true;
    }
    ccz::run_chunk(h, "als", "n_sweeps", S, n_sweeps, sweeps_known, stopped_known, &ccz::AlsStatus::total,
                   [&] {
                     const ccz::AlsViews vw = ccz::make_views(S, views, means_dev);
                     for (int i = 0; i < S.M; ++i) S.last_cs[i] = vw.cs[i];
                     return vw;
                   },
                   [&](const ccz::AlsViews& vw, int64_t) { ccz::enqueue_sweep(h, S, vw); });
  })
}

int ccz_als_status(ccz_handle h, void* state, int* dims_done, int* stopped, int64_t* sweeps_per_dim, double* last_delta) {
  CCZ_GUARD(h, {
    ccz::AlsState& S = *ccz::as_state<ccz::AlsState>("als", state);
    ccz::AlsStatus st;
    ccz::d2h(h, &st, S.drv.dev, sizeof(st));
    if (dims_done) *dims_done = st.dim;
    if (stopped) *stopped = st.stopped;
    for (int64_t d = 0; d < S.k; ++d) {
      if (sweeps_per_dim) sweeps_per_dim[d] = st.iters[d];
      if (last_delta) last_delta[d] = st.last_delta[d];
    }
  })
}

int ccz_als_colmeans(ccz_handle h, int dtype, const ccz_view* view, int64_t n_rows, void* mean_dev) {
  CCZ_GUARD(h, {
    if (!view || !view->data || !mean_dev || n_rows < 1 || view->cols < 1 || view->ld < view->cols) ccz::fail(CCZ_EINVAL, "als: bad argument");
    ccz::check_dtype("als", dtype);
    const dim3 grid(unsigned((view->cols + 255) / 256));
    ccz::by_dtype(dtype, [&](auto t) {
      using T = decltype(t);
      hipLaunchKernelGGL((ccz::k_als_colmeans<T>), grid, dim3(256), 0, ccz::stream(h), static_cast<const T*>(view->data), view->ld,
                         view->cols, n_rows, static_cast<T*>(mean_dev));
    });
    CCZ_LAUNCH_CHECK();
  })
}

int ccz_sparse_group(int64_t nnz, int64_t lines) { return (nnz < 0 || lines < 1) ? CCZ_EINVAL : ccz::sparse_group(nnz, lines); }

int ccz_als_set_sparse(ccz_handle h, void* state, int view, const ccz_sparse_view* sparse) {
  CCZ_GUARD(h, {
    ccz::AlsState& S = *ccz::as_state<ccz::AlsState>("als", state);
    if (view < 0 || view >= S.M) ccz::fail(CCZ_EINVAL, "als: no view %d", view);
    if (S.rule == ccz::RULE_ADMM || S.rule == ccz::RULE_ENET)
      ccz::fail(CCZ_EUNSUP, "als: the ADMM and elastic-net rules need the Gram of a view and take no sparse views");
    if (sparse) {
      ccz::check_sparse(sparse, true, true);
      if (sparse->rows != S.n || sparse->cols != S.p[view])
        ccz::fail(CCZ_EINVAL, "als: sparse view %d is %lld x %lld, the fit state %lld x %lld", view, (long long)sparse->rows,
                  (long long)sparse->cols, (long long)S.n, (long long)S.p[view]);
      S.sp[view] = *sparse;
      S.grow[view] = ccz::sparse_group(sparse->nnz, sparse->rows);
      S.gcol[view] = ccz::sparse_group(sparse->nnz, sparse->cols);
    }
    S.sparse[view] = sparse != nullptr;
    S.any_sparse = false;
    for (int i = 0; i < S.M; ++i) S.any_sparse = S.any_sparse || S.sparse[i];
  })
}

int ccz_sparse_colmeans(ccz_handle h, int dtype, const ccz_sparse_view* view, double* mean_dev) {
  CCZ_GUARD(h, {
    ccz::check_dtype("sparse", dtype);
    ccz::check_sparse(view, false, true);
    if (!mean_dev) ccz::fail(CCZ_EINVAL, "sparse: null argument");
    const int G = ccz::sparse_group(view->nnz, view->cols);
    ccz::by_dtype(dtype, [&](auto t) {
      using T = decltype(t);
      hipLaunchKernelGGL((ccz::k_sparse_colmeans<T>), dim3(ccz::sparse_grid(view->cols, G)), dim3(256), 0, ccz::stream(h),
                         static_cast<const T*>(view->csc_val), view->csc_ptr, view->cols, G, view->rows, mean_dev);
    });
    CCZ_LAUNCH_CHECK();
  })
}

int ccz_sparse_project(ccz_handle h, int dtype, const ccz_sparse_view* view, const double* mean_dev, const double* W_dev, int k,
                       double* out_dev) {
  CCZ_GUARD(h, {
    ccz::check_dtype("sparse", dtype);
    ccz::check_sparse(view, true, false);
    if (!W_dev || !out_dev) ccz::fail(CCZ_EINVAL, "sparse: null argument");
    if (k < 1 || k > ccz::ALS_MAXK) ccz::fail(CCZ_EUNSUP, "sparse: 1 to %d columns are supported, got %d", ccz::ALS_MAXK, k);
    ccz::DBuf muW(h, mean_dev ? k : 0);
    if (mean_dev) {
      hipLaunchKernelGGL(ccz::k_sparse_muw, dim3(k), dim3(256), 0, ccz::stream(h), mean_dev, W_dev, view->cols, k, muW.get());
      CCZ_LAUNCH_CHECK();
    }
    const int G = ccz::sparse_group(view->nnz, view->rows);
    ccz::by_dtype(dtype, [&](auto t) {
      using T = decltype(t);
      hipLaunchKernelGGL((ccz::k_sparse_project<T>), dim3(ccz::sparse_grid(view->rows, G)), dim3(256), 0, ccz::stream(h),
                         static_cast<const T*>(view->csr_val), view->csr_col, view->csr_ptr, view->rows, G, W_dev, k, muW.get(), out_dev);
    });
    CCZ_LAUNCH_CHECK();
  })
}

int ccz_als_peek(ccz_handle h, void* state, int what, int view, double* out_host) {
  CCZ_GUARD(h, {
    ccz::AlsState& S = *ccz::as_state<ccz::AlsState>("als", state);
    const ccz::AlsBuf& B = S.B;
    if (!out_host || view < 0 || view >= S.M) ccz::fail(CCZ_EINVAL, "als: bad argument");
    int64_t off = 0;
    for (int i = 0; i < view; ++i) off += S.p[i];
    const int64_t n = S.n, p = S.p[view];
    switch (what) {
      case CCZ_ALS_PEEK_Z:      // z_i and w_i coincide between iterations
      case CCZ_ALS_PEEK_W: ccz::d2h(h, out_host, B.w + off, size_t(p) * 8); break;
      case CCZ_ALS_PEEK_RAW: ccz::d2h(h, out_host, B.raw + off, size_t(p) * 8); break;
      case CCZ_ALS_PEEK_TARGET: ccz::d2h(h, out_host, B.tt, size_t(n) * 8); break;
      case CCZ_ALS_PEEK_Q: ccz::d2h(h, out_host, B.Q + int64_t(view) * S.k * n, size_t(S.k) * n * 8); break;
      case CCZ_ALS_PEEK_LEVEL: ccz::d2h(h, out_host, B.thr + 2 * view, 16); break;
      case CCZ_ALS_PEEK_ETA:
      case CCZ_ALS_PEEK_LIPSCHITZ:
        if (S.rule != ccz::RULE_ADMM) ccz::fail(CCZ_EINVAL, "als: buffer %d exists for CCZ_ALS_ADMM only", what);
        if (what == CCZ_ALS_PEEK_ETA) ccz::d2h(h, out_host, B.eta + off, size_t(p) * 8);
        else ccz::d2h(h, out_host, B.lip + view, 8);
        break;
      case CCZ_ALS_PEEK_GRAM:
      case CCZ_ALS_PEEK_RESIDUAL:
      case CCZ_ALS_PEEK_COEF:
      case CCZ_ALS_PEEK_ENET:
        if (S.rule != ccz::RULE_ENET) ccz::fail(CCZ_EINVAL, "als: buffer %d exists for CCZ_ALS_ENET only", what);
        if (what == CCZ_ALS_PEEK_GRAM) ccz::d2h(h, out_host, S.admm[view].G, size_t(p) * p * 8);
        else if (what == CCZ_ALS_PEEK_RESIDUAL) ccz::d2h(h, out_host, B.res, size_t(p) * 8);
        else if (what == CCZ_ALS_PEEK_COEF) ccz::d2h(h, out_host, B.coef + off, size_t(p) * 8);
        else ccz::d2h(h, out_host, B.scal + 4 * view, 32);
        break;
      case CCZ_ALS_PEEK_SCORE: {
        // the column-split partial sums, added in split order as the device adds them; the split count is that of the
        // last ccz_als_sweeps call
        std::vector<double> part(size_t(B.csmax) * n);
        ccz::d2h(h, part.data(), B.spart + int64_t(view) * B.csmax * n, part.size() * 8);
        const int cs = S.last_cs[view] > 0 ? S.last_cs[view] : 1;
        for (int64_t r = 0; r < n; ++r) {
          double v = 0.0;
          for (int c = 0; c < cs; ++c) v += part[size_t(c) * n + r];
          out_host[r] = v;
        }
        break;
      }
      default: ccz::fail(CCZ_EINVAL, "als: unknown buffer %d", what);
    }
  })
}

int ccz_als_get_weights(ccz_handle h, void* state, double* W_host) {
  CCZ_GUARD(h, {
    ccz::AlsState& S = *ccz::as_state<ccz::AlsState>("als", state);
    if (!W_host) ccz::fail(CCZ_EINVAL, "null argument");
    ccz::d2h(h, W_host, S.B.Wout, size_t(S.B.ptot) * S.k * 8);
  })
}

}  // extern "C"
