// The fused residual kernel of the probabilistic CCA models (svi.hip: VariationalBayesCCA; nuts.hip: ProbabilisticCCA) and its
// launch plan.  ONE read of a view X_i: a tile is a strip of 256 columns x a chunk of rc rows; R = fl(x - mu) - Z W_i' is formed per
// tile, scaled to D = R o exp(-2 s), and contracted both ways: D' Z summed over the chunk's rows (one partial per row chunk),
// D W_i summed over the strip's columns (one partial per strip), and sum R^2 exp(-2 s) per column (one partial per row chunk).
// No floating-point atomics; the including family folds the partials in index order.
//
// The kernel runs on v_mfma_f64_16x16x4f64 when K exceeds 4 (lane maps as in gfa.hip: A operand m = lane & 15, k = lane >> 4;
// B operand k = lane >> 4, n = lane & 15; C/D col = lane & 15, row = (lane >> 4) + 4 reg), on plain FMAs below.  In the MFMA form
// R is produced with its rows on the C rows and its features on the lanes, which is the A operand of D' Z as it stands; D W
// contracts over the features, so the tile goes through LDS once to put them on the contraction index.
//
// Precision: x - mu is rounded in the views' precision, then widened; every product and sum is fp64.
#pragma once

#include <algorithm>

#include "hip_common.h"
#include "fit_driver.h"
#include "reduce.h"
#include "row_load.h"

namespace ccz {

constexpr int SVI_MAXV = 8;
constexpr int SVI_MAXK = 32;
constexpr int SVI_PLAIN_K = 4;          // K up to which the fused kernel runs on plain FMAs
constexpr int SVI_SW = 256;             // columns of a strip
constexpr int SVI_MAXCHUNK = 512;       // most row chunks of the fused kernel
constexpr int64_t SVI_WANT_TILES = 8192;   // tiles (strip x row chunk) the plan aims for

typedef double v4f64 __attribute__((ext_vector_type(4)));

struct SviViews {
  const void* X[SVI_MAXV];
  const void* mu[SVI_MAXV];
  int64_t ld[SVI_MAXV];
  int64_t p[SVI_MAXV];
  int64_t off[SVI_MAXV];     // offset of view i in the concatenated rows of W and entries of s
  int ns[SVI_MAXV];          // strips of view i
  int soff[SVI_MAXV];        // index of its first strip among all strips
};

// the planned launch: nchunk row chunks of rc rows, NS strips in all; the partials are
//   wpart    nchunk x ptot x K: row-chunk partial sums of D' Z
//   s2part   nchunk x ptot: row-chunk partial sums of R^2 exp(-2 s)
//   zpart    NS x n x K: strip partial sums of D W
struct FusedPlan {
  int64_t ptot;
  int n, K, nchunk, rc, NS;
};

// the strips of every view and the row chunks: enough tiles to fill the device; a chunk holds a multiple of 16 rows and at
// least 4 K, which keeps the D' Z partials (nchunk x ptot x K doubles) at or below 2 n ptot bytes
inline void fused_plan(const char* fam, int M, const int64_t* p, int64_t n, int64_t k, SviViews& sh, FusedPlan& P) {
  P.ptot = 0;
  P.NS = 0;
  P.n = int(n);
  P.K = int(k);
  for (int i = 0; i < M; ++i) {
    sh.p[i] = p[i];
    sh.off[i] = P.ptot;
    P.ptot += p[i];
    sh.ns[i] = int((p[i] + SVI_SW - 1) / SVI_SW);
    sh.soff[i] = P.NS;
    P.NS += sh.ns[i];
  }
  if (P.ptot > (int64_t(1) << 31)) fail(CCZ_EUNSUP, "%s: at most 2^31 columns in all", fam);
  const int64_t want = std::max<int64_t>(1, std::min<int64_t>(SVI_MAXCHUNK, (SVI_WANT_TILES + P.NS - 1) / P.NS));
  int64_t rc = std::max<int64_t>((n + want - 1) / want, std::max<int64_t>(16, 4 * k));
  rc = (rc + 15) / 16 * 16;
  P.rc = int(rc);
  P.nchunk = int((n + rc - 1) / rc);
}

// plain: grid (ceil(ns / 4), nchunk), 256 threads; wave w owns strip 4 bx + w on its own (no workgroup barrier), lane l the four
// columns 256 strip + 4 l .. + 3, over rows [rc by, rc (by + 1)).  wpart / s2part point at the view's first column of chunk 0,
// zpart at the view's first strip.
template <typename T, typename St>
__global__ void __launch_bounds__(256) k_svi_fused_plain(const T* __restrict__ X, const T* __restrict__ mu, int64_t ld, int64_t p, int n,
                                                        int rc, int K, int64_t ptot, const double* __restrict__ tw,
                                                        const double* __restrict__ ts, const double* __restrict__ tz,
                                                        double* __restrict__ wpart, double* __restrict__ s2part,
                                                        double* __restrict__ zpart, const St* st) {
  if (fit_stopped(st)) return;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int64_t strip = int64_t(blockIdx.x) * 4 + wave;
  if (strip * SVI_SW >= p) return;
  const int64_t f0 = strip * SVI_SW + 4 * lane;
  const int r0 = blockIdx.y * rc, r1 = min(n, r0 + rc);
  const bool vec = vec_ok(X, ld, mu);
  T m[4] = {T(0), T(0), T(0), T(0)};
  if (mu && f0 < p) load4<T>(mu, f0, p, vec, m);
  double w[4][SVI_PLAIN_K], acc[4][SVI_PLAIN_K], e2[4], s2[4];
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const bool live = f0 + q < p;
    e2[q] = live ? exp(-2.0 * ts[f0 + q]) : 0.0;
    s2[q] = 0.0;
#pragma unroll
    for (int a = 0; a < SVI_PLAIN_K; ++a) {
      w[q][a] = (live && a < K) ? tw[(f0 + q) * K + a] : 0.0;
      acc[q][a] = 0.0;
    }
  }
  double keep[SVI_PLAIN_K] = {0.0, 0.0, 0.0, 0.0};
  for (int r = r0; r < r1; ++r) {
    T x[4] = {T(0), T(0), T(0), T(0)};
    if (f0 < p) load4<T>(X + int64_t(r) * ld, f0, p, vec, x);
    double zr[SVI_PLAIN_K], t[SVI_PLAIN_K];
#pragma unroll
    for (int a = 0; a < SVI_PLAIN_K; ++a) {
      zr[a] = a < K ? tz[int64_t(r) * K + a] : 0.0;
      t[a] = 0.0;
    }
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      double R = f0 + q < p ? double(T(x[q] - m[q])) : 0.0;
#pragma unroll
      for (int a = 0; a < SVI_PLAIN_K; ++a) R -= zr[a] * w[q][a];
      const double D = R * e2[q];
      s2[q] += R * D;
#pragma unroll
      for (int a = 0; a < SVI_PLAIN_K; ++a) {
        acc[q][a] += D * zr[a];
        t[a] += D * w[q][a];
      }
    }
    const int slot = (r - r0) & 63;
#pragma unroll
    for (int a = 0; a < SVI_PLAIN_K; ++a)
      if (a < K) {
        const double s = wave_sum(t[a]);
        if (lane == slot) keep[a] = s;
      }
    if (slot == 63 || r == r1 - 1) {     // the wave's last 64 rows (or fewer), one row per lane
      const int rr = r - slot + lane;
      if (rr <= r)
#pragma unroll
        for (int a = 0; a < SVI_PLAIN_K; ++a)
          if (a < K) zpart[(strip * n + rr) * K + a] = keep[a];
    }
  }
  double* wout = wpart + int64_t(blockIdx.y) * ptot * K;
  double* sout = s2part + int64_t(blockIdx.y) * ptot;
#pragma unroll
  for (int q = 0; q < 4; ++q)
    if (f0 + q < p) {
      sout[f0 + q] = s2[q];
#pragma unroll
      for (int a = 0; a < SVI_PLAIN_K; ++a)
        if (a < K) wout[(f0 + q) * K + a] = acc[q][a];
    }
}

// MFMA: grid (ns, nchunk), 256 threads; the workgroup owns strip bx, wave w its features 256 bx + 64 w .. + 63 as four groups q of 16:
// feature index i of group q is feature 4 i + q of the wave (a lane loads 4 consecutive features).  Rows go 16 at a time.
//   R_q (16 rows x 16 features) = x - Z W_q'          A = Z (m: row, k: latent), B = W_q' (k: latent, n: feature); ceil(K / 4) MFMAs
//   dW_q (16 features x 16 latent) += D_q' Z           A = D_q as the C registers hold it (m: feature = lane & 15, k: row), B = Z
//   dZ (16 rows x 16 latent) += D_q W_q                A = D_q read back from LDS (m: row, k: feature), B = W_q
// the four waves' dZ are summed in wave order through LDS and written once per 16 rows.
template <typename T, int KT, typename St>
__global__ void __launch_bounds__(256) k_svi_fused_mfma(const T* __restrict__ X, const T* __restrict__ mu, int64_t ld, int64_t p, int n,
                                                       int rc, int K, int64_t ptot, const double* __restrict__ tw,
                                                       const double* __restrict__ ts, const double* __restrict__ tz,
                                                       double* __restrict__ wpart, double* __restrict__ s2part,
                                                       double* __restrict__ zpart, const St* st) {
  if (fit_stopped(st)) return;
  __shared__ double dt[4][4][16][17];
  __shared__ double red[4][16][16 * KT + 1];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int li = lane & 15, lg = lane >> 4;
  const int64_t strip = blockIdx.x;
  const int64_t fw = strip * SVI_SW + 64 * wave;
  const int64_t f0 = fw + 4 * li;
  const int r0 = blockIdx.y * rc, r1 = min(n, r0 + rc);
  const bool vec = vec_ok(X, ld, mu);
  T m[4] = {T(0), T(0), T(0), T(0)};
  if (mu && f0 < p) load4<T>(mu, f0, p, vec, m);
  double wb[4][4 * KT];        // B operand of R: W[feature 4 li + q][latent lg + 4 j]
  double wa[4][4][KT];         // B operand of dZ: W[feature 4 (lg + 4 jp) + q][latent 16 kt + li]
  double e2[4], s2[4];
  v4f64 acc[4][KT];
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const bool live = f0 + q < p;
    e2[q] = live ? exp(-2.0 * ts[f0 + q]) : 0.0;
    s2[q] = 0.0;
#pragma unroll
    for (int j = 0; j < 4 * KT; ++j) wb[q][j] = (live && lg + 4 * j < K) ? tw[(f0 + q) * K + lg + 4 * j] : 0.0;
#pragma unroll
    for (int jp = 0; jp < 4; ++jp) {
      const int64_t f = fw + 4 * (lg + 4 * jp) + q;
#pragma unroll
      for (int kt = 0; kt < KT; ++kt) wa[q][jp][kt] = (f < p && 16 * kt + li < K) ? tw[f * K + 16 * kt + li] : 0.0;
    }
#pragma unroll
    for (int kt = 0; kt < KT; ++kt) acc[q][kt] = v4f64{0.0, 0.0, 0.0, 0.0};
  }
  for (int rb = r0; rb < r1; rb += 16) {
    v4f64 C[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) C[q] = v4f64{0.0, 0.0, 0.0, 0.0};
#pragma unroll
    for (int j = 0; j < 4 * KT; ++j) {
      if (4 * j >= K) break;
      const double za = (rb + li < r1 && lg + 4 * j < K) ? tz[int64_t(rb + li) * K + lg + 4 * j] : 0.0;
#pragma unroll
      for (int q = 0; q < 4; ++q) C[q] = __builtin_amdgcn_mfma_f64_16x16x4f64(za, wb[q][j], C[q], 0, 0, 0);
    }
    double D[4][4];
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      const int row = rb + lg + 4 * g;
      const bool live = row < r1;
      T x[4] = {T(0), T(0), T(0), T(0)};
      if (live && f0 < p) load4<T>(X + int64_t(row) * ld, f0, p, vec, x);
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const double R = (live && f0 + q < p) ? double(T(x[q] - m[q])) - C[q][g] : 0.0;
        D[q][g] = R * e2[q];
        s2[q] += R * D[q][g];
      }
    }
#pragma unroll
    for (int kt = 0; kt < KT; ++kt) {
      if (16 * kt >= K) break;
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        const int row = rb + lg + 4 * g;
        const double zb = (row < r1 && 16 * kt + li < K) ? tz[int64_t(row) * K + 16 * kt + li] : 0.0;
#pragma unroll
        for (int q = 0; q < 4; ++q) acc[q][kt] = __builtin_amdgcn_mfma_f64_16x16x4f64(D[q][g], zb, acc[q][kt], 0, 0, 0);
      }
    }
#pragma unroll
    for (int q = 0; q < 4; ++q)
#pragma unroll
      for (int g = 0; g < 4; ++g) dt[wave][q][lg + 4 * g][li] = D[q][g];
    __syncthreads();
    v4f64 dz[KT];
#pragma unroll
    for (int kt = 0; kt < KT; ++kt) dz[kt] = v4f64{0.0, 0.0, 0.0, 0.0};
#pragma unroll
    for (int q = 0; q < 4; ++q)
#pragma unroll
      for (int jp = 0; jp < 4; ++jp) {
        const double da = dt[wave][q][li][lg + 4 * jp];
#pragma unroll
        for (int kt = 0; kt < KT; ++kt) {
          if (16 * kt >= K) break;
          dz[kt] = __builtin_amdgcn_mfma_f64_16x16x4f64(da, wa[q][jp][kt], dz[kt], 0, 0, 0);
        }
      }
#pragma unroll
    for (int kt = 0; kt < KT; ++kt)
#pragma unroll
      for (int g = 0; g < 4; ++g) red[wave][lg + 4 * g][16 * kt + li] = dz[kt][g];
    __syncthreads();
    for (int e = threadIdx.x; e < 16 * 16 * KT; e += 256) {
      const int rr = e / (16 * KT), col = e % (16 * KT);
      const int row = rb + rr;
      if (row < r1 && col < K) zpart[(strip * n + row) * K + col] = ((red[0][rr][col] + red[1][rr][col]) + red[2][rr][col]) + red[3][rr][col];
    }
  }
  double* wout = wpart + int64_t(blockIdx.y) * ptot * K;
  double* sout = s2part + int64_t(blockIdx.y) * ptot;
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    double v = s2[q];
    v += __shfl_xor(v, 16, 64);
    v += __shfl_xor(v, 32, 64);
    if (lg == 0 && f0 + q < p) sout[f0 + q] = v;
#pragma unroll
    for (int kt = 0; kt < KT; ++kt) {
      const int col = 16 * kt + li;
      if (col >= K) continue;
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        const int64_t f = fw + 4 * (lg + 4 * g) + q;
        if (f < p) wout[f * K + col] = acc[q][kt][g];
      }
    }
  }
}

// view i through the fused kernel: W (ptot x K), s (ptot) and Z (n x K) are the sites of ALL views in the flat layout, the
// partials those of the plan; st is the family's device status word
template <typename T, typename St>
void launch_fused(ccz_ctx* c, const FusedPlan& P, const SviViews& vw, int i, const double* W, const double* s, const double* Z,
                  double* wpart_all, double* s2part_all, double* zpart_all, const St* st) {
  const T* X = static_cast<const T*>(vw.X[i]);
  const T* mu = static_cast<const T*>(vw.mu[i]);
  const double* tw = W + vw.off[i] * P.K;
  const double* ts = s + vw.off[i];
  const double* tz = Z;
  double* wpart = wpart_all + vw.off[i] * P.K;
  double* s2part = s2part_all + vw.off[i];
  double* zpart = zpart_all + int64_t(vw.soff[i]) * P.n * P.K;
  if (P.K <= SVI_PLAIN_K) {
    const dim3 grid(unsigned((vw.ns[i] + 3) / 4), unsigned(P.nchunk));
    hipLaunchKernelGGL((k_svi_fused_plain<T, St>), grid, dim3(256), 0, stream(c), X, mu, vw.ld[i], vw.p[i], P.n, P.rc, P.K, P.ptot, tw, ts, tz,
                       wpart, s2part, zpart, st);
  } else {
    const dim3 grid(unsigned(vw.ns[i]), unsigned(P.nchunk));
    if (P.K <= 16)
      hipLaunchKernelGGL((k_svi_fused_mfma<T, 1, St>), grid, dim3(256), 0, stream(c), X, mu, vw.ld[i], vw.p[i], P.n, P.rc, P.K, P.ptot, tw, ts, tz,
                         wpart, s2part, zpart, st);
    else
      hipLaunchKernelGGL((k_svi_fused_mfma<T, 2, St>), grid, dim3(256), 0, stream(c), X, mu, vw.ld[i], vw.p[i], P.n, P.rc, P.K, P.ptot, tw, ts, tz,
                         wpart, s2part, zpart, st);
  }
  CCZ_LAUNCH_CHECK();
}

}  // namespace ccz
