// Eckart-Young gradient models (CCA_EY / PLS_EY / MCCA_EY): mini-batch momentum SGD on the device.
//
// Reference: cca_zoo/linear/gradient/_base.py:101-130 (the loop), _cca_ey.py:183-225 (_derivative / _objective),
// cca_zoo/_utils/_ey.py:36-61 (ey_cross_covariance), :85-96 (weight_gram_mean).  Per step, for M views of widths p_i,
// a mini-batch of bs gathered rows X_b and weights W_i (p_i x k):
//   Z_i = (X_i[idx] - mu_i) W_i                                              launch 1  k_ey_project
//   zbar_i = mean_r Z_i,  Zt_i = Z_i - zbar_i,  V = sum_i Zt_i'Zt_i / (M (bs - 1)),
//   tr C = sum_r |sum_i Zt_i[r]|^2 / (M (bs - 1)),  v_blend = (1 - c) V + c B(W),
//   reward = -2 (tr C - c tr V)                                              launch 2  k_ey_moments (one workgroup)
//   T_i = 4 / (M (bs - 1)) (c Zt_i + (1 - c) Zt_i v_blend - sum_j Zt_j),
//   G_i = (X_i[idx] - mu_i)' T_i + (4 c / M) W_i v_blend,  vel = momentum vel - lr G,  W_i += vel,
//   per-workgroup partial sums of W_new' W_new                               launch 3  k_ey_update
//   B(W_new) = sum_i W_i'W_i / M,  obj = reward + tr(v_obj v_obj), v_obj = (1 - c) V + c B(W_new);
//   stop when |prev - obj| < tol (prev = inf at the start), steps += 1      launch 4  k_ey_finish (one workgroup)
// Every launch of a later step reads the stop word first and returns at once; the host never waits inside a chunk.
// The reference's view_c' z_term equals X_b' z_term exactly in maths (z_term's columns sum to zero), so the batch is
// never re-centred: mu (the GLOBAL mean, input precision) is subtracted on load -- fl32(x - mu32) for fp32 views,
// the same rounding as the reference's own `v - m` (cca_zoo/_base.py:97-99).
//
// Precision: fp64 views go through v_mfma_f64_16x16x4f64 end to end.  fp32 views go through v_mfma_f32_16x16x4f32:
// centred fp32 rows times W (or T) rounded to fp32, accumulated in fp32 over one stage (<= 1024 features in launch 1,
// 32 rows in launch 3) and summed in fp64 across stages.  W, the velocity and all k x k algebra stay fp64.
//
// MFMA lane maps (16x16x4): A operand lane l holds A[l & 15][l >> 4], B operand B[l >> 4][l & 15]; C/D column l & 15,
// row 4 (l >> 4) + r (f32) or (l >> 4) + 4 r (f64) in register r.
// k_ey_project: 4 waves split the features of a 32-row tile; each lane loads 4 consecutive features of one row
//   (feature f = 4 (l >> 4) + q of a 16-feature slice feeds MFMA q), W is read with the same map.
// k_ey_update: wave w owns 16 Q consecutive features; lane l loads features 4 (l & 15) .. +Q-1 of one batch row, so
//   MFMA q accumulates G rows {Q i + q}.  T (32 batch rows x k) is formed in LDS by the whole workgroup per stage.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <vector>

#include "hip_common.h"
#include "abi_guard.h"
#include "fit_driver.h"
#include "row_load.h"

namespace ccz {

namespace {

typedef float v4f32 __attribute__((ext_vector_type(4)));
typedef double v4f64 __attribute__((ext_vector_type(4)));

constexpr int EY_MAXV = 16;        // views per fit (kernel argument arrays)
constexpr int EY_ROWS = 32;        // launch 1: batch rows per workgroup (two 16-row MFMA tiles)
constexpr int EY_FOLD = 64;        // launch 1: 16-feature slices per fp32 stage before the fp64 fold
constexpr int EY_TROWS = 32;       // launch 3: batch rows per T stage

struct EyViews {
  const void* X[EY_MAXV];
  const void* mu[EY_MAXV];
  int64_t ld[EY_MAXV];
  int64_t p[EY_MAXV];
  int64_t woff[EY_MAXV];           // offset of view i's block in W (elements): k sum_{j<i} p_j
  int nblk[EY_MAXV];               // launch 3 workgroups that own columns of view i
};

// device-resident fit status, written only by k_ey_finish
struct EyStatus {
  double prev_obj;
  double last_obj;
  long long steps;
  int stopped;
  int pad;
};

// the small fp64 scratch of one step (k x k blocks, per-view means, the reward)
struct EyScratch {
  double* zmean;    // M x k
  double* V;        // k x k
  double* vblend;   // k x k
  double* B;        // k x k: B of the CURRENT weights
  double* reward;   // 1
};

template <typename T> struct Mfma;
template <> struct Mfma<float> {
  typedef v4f32 acc_t;
  __device__ static acc_t op(float a, float b, acc_t c) { return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0); }
  __device__ static int row(int lane, int r) { return 4 * (lane >> 4) + r; }
};
template <> struct Mfma<double> {
  typedef v4f64 acc_t;
  __device__ static acc_t op(double a, double b, acc_t c) { return __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, c, 0, 0, 0); }
  __device__ static int row(int lane, int r) { return (lane >> 4) + 4 * r; }
};

// x - mu in the input precision (no centring when mu is null)
template <typename T>
__device__ __forceinline__ T ey_load(const T* row, const T* mu, int64_t f, int64_t p) {
  if (f >= p) return T(0);
  return mu ? T(row[f] - mu[f]) : row[f];
}

// x[t][q] = row_t[f0 + q] - mu[f0 + q] (zero beyond p or for dead rows); one or two 16-byte loads per row when `vec` (vec_ok)
template <typename T, int NR>
__device__ __forceinline__ void ey_load4(const T* const* rowp, const bool* live, const T* mu, int64_t f0, int64_t p, bool vec,
                                         T (*x)[4]) {
#pragma unroll
  for (int t = 0; t < NR; ++t) {
    if (vec && live[t] && f0 + 3 < p) {
      T v[4], m[4] = {T(0), T(0), T(0), T(0)};
      ld4(rowp[t] + f0, v);
      if (mu) ld4(mu + f0, m);
#pragma unroll
      for (int q = 0; q < 4; ++q) x[t][q] = mu ? T(v[q] - m[q]) : v[q];
    } else {
#pragma unroll
      for (int q = 0; q < 4; ++q) x[t][q] = live[t] ? ey_load(rowp[t], mu, f0 + q, p) : T(0);
    }
  }
}

// ---- launch 1: Z_i (bs x k, fp64) = (X_i[idx] - mu_i) W_i ------------------------------------------------------------
// grid (ceil(bs / 32), M), 256 threads.  Wt: the weights in the input precision (fp32 copy for fp32 views).
template <typename T, int KT>
__global__ void __launch_bounds__(256) k_ey_project(EyViews vw, const T* __restrict__ Wt, int64_t k, const int* __restrict__ idx,
                                                   int64_t bs, double* __restrict__ Z, const EyStatus* st) {
  if (st && fit_stopped(st)) return;
  typedef typename Mfma<T>::acc_t acc_t;
  __shared__ double red[4][EY_ROWS][16];
  const int v = blockIdx.y;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int64_t p = vw.p[v], ld = vw.ld[v];
  const T* X = static_cast<const T*>(vw.X[v]);
  const T* mu = static_cast<const T*>(vw.mu[v]);
  const T* W = Wt + vw.woff[v];
  const int64_t r0 = int64_t(blockIdx.x) * EY_ROWS;
  const int g = lane >> 4, li = lane & 15;
  const T* rowp[2];
  bool live[2];
#pragma unroll
  for (int t = 0; t < 2; ++t) {
    const int64_t r = r0 + 16 * t + li;
    live[t] = r < bs;
    const int64_t src = live[t] ? (idx ? int64_t(idx[r]) : r) : 0;
    rowp[t] = X + src * ld;
  }
  acc_t acc[2][KT];
  double sum[2][KT][4];
#pragma unroll
  for (int t = 0; t < 2; ++t)
#pragma unroll
    for (int kt = 0; kt < KT; ++kt) {
      acc[t][kt] = acc_t{0, 0, 0, 0};
#pragma unroll
      for (int r = 0; r < 4; ++r) sum[t][kt][r] = 0.0;
    }
  const bool vec = vec_ok(X, ld, mu);
  const int64_t nslice = (p + 15) / 16;
  int staged = 0;
  for (int64_t s = wave; s < nslice; s += 4) {
    const int64_t f0 = 16 * s + 4 * g;
    T x[2][4];
    ey_load4<T, 2>(rowp, live, mu, f0, p, vec, x);
#pragma unroll
    for (int kt = 0; kt < KT; ++kt) {
      const int64_t col = 16 * kt + li;
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int64_t f = f0 + q;
        const T w = (f < p && col < k) ? W[f * k + col] : T(0);
#pragma unroll
        for (int t = 0; t < 2; ++t) acc[t][kt] = Mfma<T>::op(x[t][q], w, acc[t][kt]);
      }
    }
    if (++staged == EY_FOLD) {
      staged = 0;
#pragma unroll
      for (int t = 0; t < 2; ++t)
#pragma unroll
        for (int kt = 0; kt < KT; ++kt) {
#pragma unroll
          for (int r = 0; r < 4; ++r) sum[t][kt][r] += double(acc[t][kt][r]);
          acc[t][kt] = acc_t{0, 0, 0, 0};
        }
    }
  }
  // reduce the four waves' partial tiles in fp64, one 16-column tile at a time
#pragma unroll
  for (int kt = 0; kt < KT; ++kt) {
#pragma unroll
    for (int t = 0; t < 2; ++t)
#pragma unroll
      for (int r = 0; r < 4; ++r) red[wave][16 * t + Mfma<T>::row(lane, r)][li] = sum[t][kt][r] + double(acc[t][kt][r]);
    __syncthreads();
    for (int e = threadIdx.x; e < EY_ROWS * 16; e += 256) {
      const int rr = e >> 4, cc = e & 15;
      const int64_t r = r0 + rr, col = 16 * kt + cc;
      if (r < bs && col < k) Z[(int64_t(v) * bs + r) * k + col] = red[0][rr][cc] + red[1][rr][cc] + red[2][rr][cc] + red[3][rr][cc];
    }
    __syncthreads();
  }
}

// ---- launch 2: batch means, V, v_blend, the reward part of the objective (one workgroup) ---------------------------
// 32 lanes (one half-wave) share one entry and split the rows; the partial sums meet through shuffles
__device__ __forceinline__ double ey_half_sum(double v) {
#pragma unroll
  for (int o = 16; o > 0; o >>= 1) v += __shfl_xor(v, o, 32);
  return v;
}

__global__ void __launch_bounds__(1024) k_ey_moments(const double* __restrict__ Z, int M, int64_t bs, int64_t k, double c,
                                                    EyScratch s, const EyStatus* st) {
  if (fit_stopped(st)) return;
  __shared__ double part[32];
  const int tid = threadIdx.x, sl = tid & 31, grp = tid >> 5;   // 32 groups of 32 lanes
  const double inv_bs = 1.0 / double(bs), norm = 1.0 / (double(M) * double(bs - 1));
  for (int e0 = 0; e0 < M * k; e0 += 32) {
    const int e = e0 + grp;
    double acc = 0.0;
    if (e < M * k) {
      const int v = e / int(k), a = e % int(k);
      const double* z = Z + int64_t(v) * bs * k + a;
      for (int64_t r = sl; r < bs; r += 32) acc += z[r * k];
    }
    acc = ey_half_sum(acc);
    if (e < M * k && sl == 0) s.zmean[e] = acc * inv_bs;
  }
  __syncthreads();
  // V over the upper triangle (entry e -> (a, b), b >= a)
  const int64_t nup = k * (k + 1) / 2;
  for (int64_t e0 = 0; e0 < nup; e0 += 32) {
    const int64_t e = e0 + grp;
    int64_t a = 0, b = 0;
    double acc = 0.0;
    if (e < nup) {
      int64_t rem = e;
      while (rem >= k - a) { rem -= k - a; ++a; }
      b = a + rem;
      for (int v = 0; v < M; ++v) {
        const double* z = Z + int64_t(v) * bs * k;
        const double ma = s.zmean[v * k + a], mb = s.zmean[v * k + b];
        for (int64_t r = sl; r < bs; r += 32) acc += (z[r * k + a] - ma) * (z[r * k + b] - mb);
      }
    }
    acc = ey_half_sum(acc);
    if (e < nup && sl == 0) {
      s.V[a * k + b] = acc * norm;
      s.V[b * k + a] = acc * norm;
    }
  }
  // tr C: sum over rows of |sum_i Zt_i[r]|^2, one (row, column) element per thread at a time
  double tc = 0.0;
  for (int64_t e = tid; e < bs * k; e += 1024) {
    const int64_t a = e % k;
    double t = 0.0;
    for (int v = 0; v < M; ++v) t += Z[int64_t(v) * bs * k + e] - s.zmean[v * k + a];
    tc += t * t;
  }
  tc = ey_half_sum(tc);
  if (sl == 0) part[grp] = tc;
  __syncthreads();
  for (int64_t e = tid; e < k * k; e += 1024) s.vblend[e] = (1.0 - c) * s.V[e] + c * s.B[e];
  if (tid == 0) {
    double tcs = 0.0, trv = 0.0;
    for (int g = 0; g < 32; ++g) tcs += part[g];
    for (int64_t a = 0; a < k; ++a) trv += s.V[a * k + a];
    s.reward[0] = -2.0 * (tcs * norm - c * trv);
  }
}

// ---- launch 3: G_i = X_b' T_i + (4c/M) W_i v_blend, momentum update, partial W_new' W_new ----------------------------
// grid (max_i nblk_i, M), 256 threads; workgroup b of view v owns features [64 Q b, 64 Q (b + 1)).  W (fp64) is read from
// Wcur and written to Wnext (double buffer: the direct term needs the old rows); Wt (input precision) receives W_new.
template <typename T, int KT, int Q>
__global__ void __launch_bounds__(256) k_ey_update(EyViews vw, const double* __restrict__ Wcur, double* __restrict__ Wnext,
                                                  double* __restrict__ vel, T* __restrict__ Wt, int64_t k,
                                                  const int* __restrict__ idx, int64_t bs, const double* __restrict__ Z,
                                                  EyScratch s, int M, double c, double lr, double mom,
                                                  double* __restrict__ Bpart, int bstride, const EyStatus* st) {
  if (fit_stopped(st)) return;
  typedef typename Mfma<T>::acc_t acc_t;
  extern __shared__ double ey_lds[];
  T* Ts = reinterpret_cast<T*>(ey_lds);                      // EY_TROWS x (16 KT)
  const int v = blockIdx.y;
  const int64_t p = vw.p[v];
  if (int(blockIdx.x) >= vw.nblk[v]) return;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int g = lane >> 4, li = lane & 15;
  const int KC = 16 * KT;
  const int64_t ld = vw.ld[v];
  const T* X = static_cast<const T*>(vw.X[v]);
  const T* mu = static_cast<const T*>(vw.mu[v]);
  const int64_t fw = int64_t(blockIdx.x) * 64 * Q + 16 * Q * wave;   // this wave's first feature
  const double scale = 4.0 / (double(M) * double(bs - 1));
  const bool vec = vec_ok(X, ld, mu);
  acc_t acc[Q][KT];
  double sum[Q][KT][4];
#pragma unroll
  for (int q = 0; q < Q; ++q)
#pragma unroll
    for (int kt = 0; kt < KT; ++kt) {
      acc[q][kt] = acc_t{0, 0, 0, 0};
#pragma unroll
      for (int r = 0; r < 4; ++r) sum[q][kt][r] = 0.0;
    }
  const double* zv = Z + int64_t(v) * bs * k;
  for (int64_t r0 = 0; r0 < bs; r0 += EY_TROWS) {
    // T rows r0 .. r0 + 31 of view v (zero beyond bs and k)
    for (int e = threadIdx.x; e < EY_TROWS * KC; e += 256) {
      const int rr = e / KC, b = e % KC;
      const int64_t r = r0 + rr;
      double t = 0.0;
      if (r < bs && b < k) {
        double zb = 0.0, tot = 0.0, mix = 0.0;
        for (int u = 0; u < M; ++u) tot += Z[(int64_t(u) * bs + r) * k + b] - s.zmean[u * k + b];
        zb = zv[r * k + b] - s.zmean[v * k + b];
        for (int64_t a = 0; a < k; ++a) mix += (zv[r * k + a] - s.zmean[v * k + a]) * s.vblend[a * k + b];
        t = scale * (c * zb + (1.0 - c) * mix - tot);
      }
      Ts[rr * KC + b] = T(t);
    }
    __syncthreads();
#pragma unroll 2
    for (int rs = 0; rs < EY_TROWS; rs += 4) {
      const int64_t r = r0 + rs + g;
      T x[Q];
      if (r < bs) {
        const T* row = X + (idx ? int64_t(idx[r]) : r) * ld;
        if constexpr (Q == 4) {
          T x4[1][4];
          const bool lv[1] = {true};
          const T* rp[1] = {row};
          ey_load4<T, 1>(rp, lv, mu, fw + Q * li, p, vec, x4);
#pragma unroll
          for (int q = 0; q < Q; ++q) x[q] = x4[0][q];
        } else {
#pragma unroll
          for (int q = 0; q < Q; ++q) x[q] = ey_load(row, mu, fw + Q * li + q, p);
        }
      } else {
#pragma unroll
        for (int q = 0; q < Q; ++q) x[q] = T(0);
      }
#pragma unroll
      for (int kt = 0; kt < KT; ++kt) {
        const T tv = Ts[(rs + g) * KC + 16 * kt + li];
#pragma unroll
        for (int q = 0; q < Q; ++q) acc[q][kt] = Mfma<T>::op(x[q], tv, acc[q][kt]);
      }
    }
#pragma unroll
    for (int q = 0; q < Q; ++q)
#pragma unroll
      for (int kt = 0; kt < KT; ++kt) {
#pragma unroll
        for (int r = 0; r < 4; ++r) sum[q][kt][r] += double(acc[q][kt][r]);
        acc[q][kt] = acc_t{0, 0, 0, 0};
      }
    __syncthreads();
  }
  // epilogue: row i of MFMA q is feature fw + Q i + q, column 16 kt + li is latent dimension b
  const int64_t wo = vw.woff[v];
  const double direct = 4.0 * c / double(M);
#pragma unroll
  for (int q = 0; q < Q; ++q)
#pragma unroll
    for (int kt = 0; kt < KT; ++kt)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int64_t f = fw + Q * Mfma<T>::row(lane, r) + q;
        const int64_t b = 16 * kt + li;
        if (f >= p || b >= k) continue;
        const double* wrow = Wcur + wo + f * k;
        double dv = 0.0;
        for (int64_t a = 0; a < k; ++a) dv += wrow[a] * s.vblend[a * k + b];
        const double grad = sum[q][kt][r] + direct * dv;
        const int64_t e = wo + f * k + b;
        const double nv = mom * vel[e] - lr * grad;
        vel[e] = nv;
        const double nw = wrow[b] + nv;
        Wnext[e] = nw;
        if (Wt) Wt[e] = T(nw);
      }
  __syncthreads();
  // partial B of this workgroup's features: sum_f W_new[f]' W_new[f]
  const int64_t f0 = int64_t(blockIdx.x) * 64 * Q;
  const int64_t f1 = f0 + 64 * Q < p ? f0 + 64 * Q : p;
  double* out = Bpart + (int64_t(v) * bstride + blockIdx.x) * k * k;
  for (int64_t e = threadIdx.x; e < k * k; e += 256) {
    const int64_t a = e / k, b = e % k;
    double acc2 = 0.0;
    for (int64_t f = f0; f < f1; ++f) acc2 += Wnext[wo + f * k + a] * Wnext[wo + f * k + b];
    out[e] = acc2;
  }
}

// ---- launch 4: B(W_new), the objective, the stop test (one workgroup) -----------------------------------------------
__global__ void __launch_bounds__(256) k_ey_finish(EyViews vw, const double* __restrict__ Bpart, int bstride, int M, int64_t k,
                                                  double c, double tol, EyScratch s, EyStatus* st, long long step) {
  if (fit_stopped(st)) return;
  __shared__ double part[256];
  const int tid = threadIdx.x;
  double tr = 0.0;
  for (int64_t e = tid; e < k * k; e += 256) {
    double acc = 0.0;
    for (int v = 0; v < M; ++v)
      for (int b = 0; b < vw.nblk[v]; ++b) acc += Bpart[(int64_t(v) * bstride + b) * k * k + e];
    s.B[e] = acc / double(M);
  }
  __syncthreads();
  // tr(v_obj v_obj) = sum_ab v_obj[a][b] v_obj[b][a]
  for (int64_t e = tid; e < k * k; e += 256) {
    const int64_t a = e / k, b = e % k;
    const double x = (1.0 - c) * s.V[a * k + b] + c * s.B[a * k + b];
    const double y = (1.0 - c) * s.V[b * k + a] + c * s.B[b * k + a];
    tr += x * y;
  }
  part[tid] = tr;
  __syncthreads();
  for (int w = 128; w > 0; w >>= 1) {
    if (tid < w) part[tid] += part[tid + w];
    __syncthreads();
  }
  if (tid == 0) {
    const double obj = s.reward[0] + part[0];
    const double prev = st->prev_obj;
    st->last_obj = obj;
    st->steps = step + 1;
    if (fabs(prev - obj) < tol) st->stopped = 1;   // NaN never stops (the comparison is false)
    else st->prev_obj = obj;
  }
}

// ---- host driver ----------------------------------------------------------------------------------------------------
struct EyState : FitState<EyStatus> {
  int64_t k, bs;
  double c, lr, mom, tol;
  std::vector<int64_t> woff;
  int64_t ptot;
  int Q, KT, cols_per_blk, nblk_max;
  double* W[2] = {nullptr, nullptr};
  double* vel = nullptr;
  float* Wf = nullptr;       // fp32 views: W rounded to fp32, read by the projection (fp64 views read W itself)
  double* Z = nullptr;
  double* small = nullptr;   // zmean | V | vblend | B | reward
  double* Bpart = nullptr;
  int* idx_dev[2] = {nullptr, nullptr};   // the chunk's row indices ride on the driver's slots and events
  PinMem<int> idx_pin[2];
  long long enqueued = 0;    // steps enqueued since the last set_weights
  EyScratch scratch() const {
    EyScratch s;
    s.zmean = small;
    s.V = small + M * k;
    s.vblend = s.V + k * k;
    s.B = s.vblend + k * k;
    s.reward = s.B + k * k;
    return s;
  }
};

int kt_for(int64_t k) {
  const int64_t t = (k + 15) / 16;
  return t <= 1 ? 1 : t <= 2 ? 2 : t <= 4 ? 4 : 8;
}

EyViews make_views(const EyState& S, const ccz_view* views, const void* const* means) {
  EyViews vw;
  memset(&vw, 0, sizeof(vw));
  fill_views("ey", vw, views, means, S.p);
  for (int i = 0; i < S.M; ++i) {
    vw.p[i] = S.p[i];
    vw.woff[i] = S.woff[i];
    vw.nblk[i] = int((S.p[i] + S.cols_per_blk - 1) / S.cols_per_blk);
  }
  return vw;
}

template <typename T>
void launch_project(ccz_ctx* c, const EyState& S, const EyViews& vw, const int* idx, int64_t bs, double* Z, const EyStatus* st) {
  const T* Wt;     // fp32 views read the rounded copy of the current weights
  if constexpr (sizeof(T) == 4) Wt = S.Wf;
  else Wt = S.W[int(S.enqueued & 1)];
  const dim3 grid(unsigned((bs + EY_ROWS - 1) / EY_ROWS), unsigned(S.M));
  switch (S.KT) {
    case 1: hipLaunchKernelGGL((k_ey_project<T, 1>), grid, dim3(256), 0, stream(c), vw, Wt, S.k, idx, bs, Z, st); break;
    case 2: hipLaunchKernelGGL((k_ey_project<T, 2>), grid, dim3(256), 0, stream(c), vw, Wt, S.k, idx, bs, Z, st); break;
    case 4: hipLaunchKernelGGL((k_ey_project<T, 4>), grid, dim3(256), 0, stream(c), vw, Wt, S.k, idx, bs, Z, st); break;
    default: hipLaunchKernelGGL((k_ey_project<T, 8>), grid, dim3(256), 0, stream(c), vw, Wt, S.k, idx, bs, Z, st); break;
  }
  CCZ_LAUNCH_CHECK();
}

template <typename T, int KT, int Q>
void launch_update_q(ccz_ctx* c, const EyState& S, const EyViews& vw, int cur, const int* idx) {
  T* Wt = nullptr;
  if constexpr (sizeof(T) == 4) Wt = S.Wf;
  const dim3 grid(unsigned(S.nblk_max), unsigned(S.M));
  const size_t lds = size_t(EY_TROWS) * 16 * KT * sizeof(T);
  hipLaunchKernelGGL((k_ey_update<T, KT, Q>), grid, dim3(256), lds, stream(c), vw, S.W[cur], S.W[cur ^ 1], S.vel, Wt, S.k, idx, S.bs, S.Z, S.scratch(), S.M, S.c, S.lr, S.mom, S.Bpart, S.nblk_max, S.drv.dev);
}

template <typename T>
void launch_update(ccz_ctx* c, const EyState& S, const EyViews& vw, int cur, const int* idx) {
  switch (S.KT) {
    case 1: launch_update_q<T, 1, 4>(c, S, vw, cur, idx); break;
    case 2: launch_update_q<T, 2, 4>(c, S, vw, cur, idx); break;
    case 4: launch_update_q<T, 4, 1>(c, S, vw, cur, idx); break;
    default: launch_update_q<T, 8, 1>(c, S, vw, cur, idx); break;
  }
  CCZ_LAUNCH_CHECK();
}

void enqueue_step(ccz_ctx* c, EyState& S, const EyViews& vw, const int* idx) {
  const int cur = int(S.enqueued & 1);
  const EyScratch s = S.scratch();
  by_dtype(S.dtype, [&](auto t) { launch_project<decltype(t)>(c, S, vw, idx, S.bs, S.Z, S.drv.dev); });
  hipLaunchKernelGGL(k_ey_moments, dim3(1), dim3(1024), 0, stream(c), S.Z, S.M, S.bs, S.k, S.c, s, S.drv.dev);
  CCZ_LAUNCH_CHECK();
  by_dtype(S.dtype, [&](auto t) { launch_update<decltype(t)>(c, S, vw, cur, idx); });
  hipLaunchKernelGGL(k_ey_finish, dim3(1), dim3(256), 0, stream(c), vw, S.Bpart, S.nblk_max, S.M, S.k, S.c, S.tol, s, S.drv.dev,
                     (long long)S.enqueued);
  CCZ_LAUNCH_CHECK();
  ++S.enqueued;
}

EyState* ey_create(ccz_ctx* c, int dtype, int M, const int64_t* p, int64_t k, int64_t bs, int64_t chunk, double cc, double lr,
                   double mom, double tol) {
  check_dtype("ey", dtype);
  check_view_count("ey", M, EY_MAXV);
  if (!p || k < 1 || k > 128 || bs < 1 || chunk < 1) fail(CCZ_EINVAL, "ey: bad argument (k must be 1..128)");
  if (bs > (int64_t(1) << 30)) fail(CCZ_EINVAL, "ey: batch too large");
  return new_state<EyState>(c, [&](EyState& S) {
    S.dtype = dtype; S.M = M; S.k = k; S.bs = bs; S.chunk = chunk;
    S.c = cc; S.lr = lr; S.mom = mom; S.tol = tol;
    S.ptot = 0;
    for (int i = 0; i < M; ++i) {
      if (p[i] < k) fail(CCZ_EINVAL, "ey: view %d has %lld features < k = %lld", i, (long long)p[i], (long long)k);
      S.p.push_back(p[i]);
      S.woff.push_back(S.ptot * k);
      S.ptot += p[i];
    }
    S.KT = kt_for(k);
    S.Q = S.KT <= 2 ? 4 : 1;
    S.cols_per_blk = 64 * S.Q;
    S.nblk_max = 0;
    for (int i = 0; i < M; ++i) S.nblk_max = std::max<int>(S.nblk_max, int((p[i] + S.cols_per_blk - 1) / S.cols_per_blk));
    const size_t wn = size_t(S.ptot * k);
    for (int i = 0; i < 2; ++i) S.W[i] = S.get(c, wn);
    S.vel = S.get(c, wn);
    if (dtype == CCZ_F32) S.Wf = S.get<float>(c, wn);
    S.Z = S.get(c, size_t(M) * bs * k);
    S.small = S.get(c, size_t(M) * k + 3 * k * k + 1);
    S.Bpart = S.get(c, size_t(M) * S.nblk_max * k * k);
    S.drv.create(c);
    for (int i = 0; i < 2; ++i) {
      S.idx_dev[i] = S.get<int>(c, size_t(chunk) * bs);
      CCZ_HIP(hipHostMalloc(S.idx_pin[i].out(), size_t(chunk) * bs * 4, hipHostMallocDefault));
    }
  });
}

void ey_set_weights(ccz_ctx* c, EyState& S, const double* W_host) {
  if (!W_host) fail(CCZ_EINVAL, "ey: null weights");
  const size_t wn = size_t(S.ptot * S.k);
  h2d(c, S.W[0], W_host, wn * 8);
  zero(c, S.vel, wn * 8);
  if (S.Wf) {
    std::vector<float> wf(W_host, W_host + wn);
    h2d(c, S.Wf, wf.data(), wn * 4);
  }
  // B of the initial weights on the host: sum_i W_i'W_i / M (cca_zoo/_utils/_ey.py:85-96)
  const int64_t k = S.k;
  std::vector<double> B(size_t(k * k), 0.0);
  for (int i = 0; i < S.M; ++i) {
    const double* w = W_host + S.woff[i];
    for (int64_t f = 0; f < S.p[i]; ++f)
      for (int64_t a = 0; a < k; ++a)
        for (int64_t b = 0; b < k; ++b) B[a * k + b] += w[f * k + a] * w[f * k + b];
  }
  for (double& x : B) x /= double(S.M);
  h2d(c, S.scratch().B, B.data(), B.size() * 8);
  EyStatus st0;
  st0.prev_obj = INFINITY;
  st0.last_obj = NAN;
  st0.steps = 0;
  st0.stopped = 0;
  st0.pad = 0;
  h2d(c, S.drv.dev, &st0, sizeof(st0));
  S.enqueued = 0;
}

// upload `rows` x bs host indices into slot `slot` (waits for the slot's previous chunk); returns the device pointer
const int* upload_idx(ccz_ctx* c, EyState& S, int slot, const int64_t* idx_host, int64_t rows, int64_t n_rows_data) {
  S.drv.wait(slot);
  int* pin = S.idx_pin[slot].get();
  for (int64_t e = 0; e < rows * S.bs; ++e) {
    const int64_t v = idx_host[e];
    if (v < 0 || v >= n_rows_data) fail(CCZ_EINVAL, "ey: row index %lld out of range [0, %lld)", (long long)v, (long long)n_rows_data);
    pin[e] = int(v);
  }
  CCZ_HIP(hipMemcpyAsync(S.idx_dev[slot], pin, size_t(rows * S.bs) * 4, hipMemcpyHostToDevice, stream(c)));
  return S.idx_dev[slot];
}

}  // namespace
}  // namespace ccz

extern "C" {

int ccz_ey_create(ccz_handle h, int dtype, int n_views, const int64_t* p, int64_t k, int64_t batch_rows, int64_t chunk_steps,
                  double c, double learning_rate, double momentum, double tol, void** state_out) {
  CCZ_GUARD(h, {
    if (!state_out) ccz::fail(CCZ_EINVAL, "null argument");
    *state_out = nullptr;
    *state_out = ccz::ey_create(h, dtype, n_views, p, k, batch_rows, chunk_steps, c, learning_rate, momentum, tol);
  })
}

int ccz_ey_destroy(ccz_handle h, void* state) {
  CCZ_GUARD(h, {
    if (state) ccz::free_state(h, static_cast<ccz::EyState*>(state));
  })
}

int ccz_ey_set_weights(ccz_handle h, void* state, const double* W_host) {
  CCZ_GUARD(h, {
    ccz::EyState& S = *ccz::as_state<ccz::EyState>("ey", state);
    S.restart(h);
    ccz::ey_set_weights(h, S, W_host);
  })
}

int ccz_ey_project(ccz_handle h, void* state, const ccz_view* views, const void* const* means_dev, int64_t n_rows,
                   const int64_t* idx_host, double* Z_host) {
  CCZ_GUARD(h, {
    ccz::EyState& S = *ccz::as_state<ccz::EyState>("ey", state);
    if (!Z_host) ccz::fail(CCZ_EINVAL, "null argument");
    if (!idx_host && n_rows != S.bs) ccz::fail(CCZ_EINVAL, "ey: without indices n_rows must equal the batch rows");
    const ccz::EyViews vw = ccz::make_views(S, views, means_dev);
    ccz::sync(h);
    const int* idx = idx_host ? ccz::upload_idx(h, S, 0, idx_host, 1, n_rows) : nullptr;
    S.drv.used[0] = false;
    ccz::by_dtype(S.dtype, [&](auto t) { ccz::launch_project<decltype(t)>(h, S, vw, idx, S.bs, S.Z, nullptr); });
    ccz::d2h(h, Z_host, S.Z, size_t(S.M) * S.bs * S.k * 8);
  })
}

int ccz_ey_steps(ccz_handle h, void* state, const ccz_view* views, const void* const* means_dev, int64_t n_rows,
                 const int64_t* idx_host, int64_t n_steps, int64_t* steps_known, int* stopped_known) {
  CCZ_GUARD(h, {
    ccz::EyState& S = *ccz::as_state<ccz::EyState>("ey", state);
    const int* idx = nullptr;
    ccz::run_chunk(h, "ey", "n_steps", S, n_steps, steps_known, stopped_known, &ccz::EyStatus::steps,
                   [&] {
                     if (!idx_host && n_rows != S.bs) ccz::fail(CCZ_EINVAL, "ey: a full-batch step needs n_rows == batch rows");
                     return ccz::make_views(S, views, means_dev);
                   },
                   [&](const ccz::EyViews& vw, int64_t t) { ccz::enqueue_step(h, S, vw, idx ? idx + t * S.bs : nullptr); },
                   [&](int slot) { if (idx_host) idx = ccz::upload_idx(h, S, slot, idx_host, n_steps, n_rows); });
  })
}

int ccz_ey_status(ccz_handle h, void* state, int64_t* steps_done, int* stopped, double* last_objective) {
  CCZ_GUARD(h, {
    ccz::EyState& S = *ccz::as_state<ccz::EyState>("ey", state);
    ccz::EyStatus st;
    ccz::d2h(h, &st, S.drv.dev, sizeof(st));
    if (steps_done) *steps_done = st.steps;
    if (stopped) *stopped = st.stopped;
    if (last_objective) *last_objective = st.last_obj;
  })
}

int ccz_ey_get_weights(ccz_handle h, void* state, double* W_host) {
  CCZ_GUARD(h, {
    ccz::EyState& S = *ccz::as_state<ccz::EyState>("ey", state);
    if (!W_host) ccz::fail(CCZ_EINVAL, "null argument");
    ccz::EyStatus st;
    ccz::d2h(h, &st, S.drv.dev, sizeof(st));
    ccz::d2h(h, W_host, S.W[int(st.steps & 1)], size_t(S.ptot * S.k) * 8);
  })
}

}  // extern "C"
