// TreeCCA: boosted-tree CCA, histogram tree growth on the device.
//
// Reference: cca_zoo/tree/_treecca.py:329-360 (the outer loop) around a histogram booster that tests/treecca_restatement.py
// specifies (xgboost's documented tree_method="hist" for the reference's parameters; no parity with xgboost's trees).
//
// Setup, per view:   k_tree_cuts     one workgroup per feature: the sampled column (at most 8192 floats = 32 KB) is sorted in LDS
//                                    (bitonic), the values at ranks j S / 256 are de-duplicated into at most 255 cut points;
//                    k_tree_bin      bin(x) = number of cuts <= x, uint8, FEATURE-major (p x n): the histogram kernel's
//                                    workgroups read one feature's column of a row chunk as contiguous bytes;
//                    k_tree_project, k_tree_colsumsq, k_tree_margin: the random-orthogonal base margin as float32.
// Gradient:          k_tree_zmom / k_tree_zfold   per-view k x k second moments and sums of the embeddings (float64 values
//                                    double(base margin) + double(float32 tree sum)), per row chunk, folded in index order;
//                    k_tree_grad     scale (Zc V - S) for every view, with per-workgroup sums of g, g^2 and max |g| per column;
//                    k_tree_gfin     the shared std, and per (view, column) the shift S = 30 - frexp_exponent(max |g32|);
//                    k_tree_quant    g32 = float(g / scale * 0.1), q = rint(g32 2^S) as int32 (|q| <= 2^30).
// Growth of the k trees of one view, level by level (d = 0 .. depth - 1), all in one set of launches:
//                    k_tree_hist     grid (row chunks of 4096, features of the tile): (int64 G, int32 H) per (component, node,
//                                    feature, bin) over the sampled rows, accumulated in LDS while k 2^d <= 16 (48 KB), flushed
//                                    with one global atomic per non-empty entry; directly in global memory below that.  Integer
//                                    atomics: the sums are exact whatever the order.
//                    k_tree_find     one workgroup per (node, component): per feature a 256-bin inclusive scan, the gain of every
//                                    admissible bin in float64 without contraction, the argmax with ties to the lower bin; the
//                                    features in ascending order, replaced only by a strictly larger gain; the running best
//                                    survives from one feature tile to the next.
//                    k_tree_commit   a node splits iff its best gain > 0: the heap arrays, the children's sums.
//                    k_tree_part     the node ids (uint8 position within the level) of ALL rows; a row under a leaf goes on to
//                                    the left (pos -> 2 pos), where no node exists and every work item passes.
//                    k_tree_leaf, k_tree_update   leaf values, the table by last-level position, T += leaf (float32).
// The histogram workspace is bounded by TREE_HIST_BYTES (64 MiB): the features of a level are tiled by
// FT = max(1, 64 MiB / (k 2^(depth - 1) 3072 B)) (at least 5 with k <= 32, depth <= 8).
// Nothing about a tree's shape comes back to the host during a fit: a round is a fixed chain of launches.
// Predict: k_tree_predict traverses raw rows against the float32 thresholds (left iff x < threshold), sums the float32 leaves
// in tree order and adds the float64 base-margin projection.
#include <algorithm>
#include <cmath>
#include <cstring>

#include "hip_common.h"
#include "abi_guard.h"
#include "fit_driver.h"
#include "reduce.h"
#include "rng_hash.h"

namespace ccz {

namespace {

constexpr int TREE_MAXK = 32, TREE_MAXDEPTH = 8, TREE_MAXVIEWS = 8, TREE_BINS = 256, TREE_CUT_SAMPLE = 8192;
constexpr int64_t TREE_MAXP = 32768, TREE_MAXN = (int64_t(1) << 31) - 1;
constexpr size_t TREE_HIST_BYTES = size_t(64) << 20;
constexpr int TREE_HROWS = 4096;                      // rows per workgroup of k_tree_hist
constexpr int TREE_LDS_ENT = 16 * TREE_BINS;          // histogram entries held in LDS (48 KB)
constexpr double TREE_TARGET_STD = 0.1;

struct TreeRec {                 // the best candidate of a (component, node) so far
  double gain;
  long long GL, G;
  int HL, H, feat, bin;
};

struct GrowBuf {
  const uint8_t* bins;           // p x n
  const float* cuts;             // p x 256 (unused entries +inf)
  const int* ncuts;              // p
  const int* q;                  // k x n
  const uint8_t* mask;           // n
  const int* flist;              // nsel, ascending
  const int* shift;              // k
  uint8_t* nid;                  // k x n
  long long* histG;              // k x 2^(depth-1) x FT x 256
  int* histH;
  TreeRec* rec;                  // k x 2^(depth-1)
  long long* nodeG;              // k x NN
  int* nodeH;
  uint8_t* state;                // k x NN: 0 no node, 1 open / leaf, 2 split
  int* feat; int* bin; float* thr; float* leaf; double* gain;   // k x NN
  float* leaftab;                // k x 2^depth
  int64_t n;
  int p, k, depth, nsel, FT, NN;
  double lr, mcw;
};

__global__ void __launch_bounds__(256) k_tree_grow_init(GrowBuf B) {
  const int64_t gt = int64_t(blockIdx.x) * 256 + threadIdx.x, gs = int64_t(gridDim.x) * 256;
  const int tot = B.k * B.NN;
  for (int64_t e = gt; e < tot; e += gs) {
    B.state[e] = (e % B.NN) == 0 ? 1 : 0;
    B.feat[e] = -1; B.bin[e] = 0; B.thr[e] = 0.0f; B.leaf[e] = 0.0f; B.gain[e] = 0.0;
    B.nodeG[e] = 0; B.nodeH[e] = 0;
  }
  const int64_t rows = int64_t(B.k) * B.n;
  for (int64_t e = gt; e < rows; e += gs) B.nid[e] = 0;
}

__global__ void __launch_bounds__(256) k_tree_hist(GrowBuf B, int d, int f0, int lds) {
  __shared__ long long lG[TREE_LDS_ENT];
  __shared__ int lH[TREE_LDS_ENT];
  const int tid = threadIdx.x, nn = 1 << d, base = nn - 1, fi = blockIdx.y;
  const int f = B.flist[f0 + fi];
  const uint8_t* __restrict__ bcol = B.bins + int64_t(f) * B.n;
  const int64_t r0 = int64_t(blockIdx.x) * TREE_HROWS, r1 = min(B.n, r0 + TREE_HROWS);
  const int ent = B.k * nn * TREE_BINS;
  if (lds) {
    for (int e = tid; e < ent; e += 256) { lG[e] = 0; lH[e] = 0; }
    __syncthreads();
  }
  for (int64_t r = r0 + tid; r < r1; r += 256) {
    if (!B.mask[r]) continue;
    const int b = bcol[r];
    for (int c = 0; c < B.k; ++c) {
      const int pos = B.nid[int64_t(c) * B.n + r];
      if (pos >= nn || B.state[c * B.NN + base + pos] != 1) continue;
      const long long qv = B.q[int64_t(c) * B.n + r];
      if (lds) {
        const int e = (c * nn + pos) * TREE_BINS + b;
        atomicAdd(reinterpret_cast<unsigned long long*>(&lG[e]), static_cast<unsigned long long>(qv));
        atomicAdd(&lH[e], 1);
      } else {
        const int64_t e = (int64_t(c * nn + pos) * B.FT + fi) * TREE_BINS + b;
        atomicAdd(reinterpret_cast<unsigned long long*>(&B.histG[e]), static_cast<unsigned long long>(qv));
        atomicAdd(&B.histH[e], 1);
      }
    }
  }
  if (lds) {
    __syncthreads();
    for (int e = tid; e < ent; e += 256) {
      if (lH[e] == 0) continue;
      const int64_t g = (int64_t(e >> 8) * B.FT + fi) * TREE_BINS + (e & 255);
      atomicAdd(reinterpret_cast<unsigned long long*>(&B.histG[g]), static_cast<unsigned long long>(lG[e]));
      atomicAdd(&B.histH[g], lH[e]);
    }
  }
}

// every operation rounded once: the restatement evaluates the same expression in NumPy
__device__ __forceinline__ double tree_gain(long long GL, int HL, long long G, int H, double sc) {
#pragma clang fp contract(off)
  const double gl = double(GL) * sc, gr = double(G - GL) * sc, g = double(G) * sc;
  const double hl = double(HL), hr = double(H - HL), h = double(H);
  const double a = __ddiv_rn(__dmul_rn(gl, gl), __dadd_rn(hl, 1.0));
  const double b = __ddiv_rn(__dmul_rn(gr, gr), __dadd_rn(hr, 1.0));
  const double t = __ddiv_rn(__dmul_rn(g, g), __dadd_rn(h, 1.0));
  return __dsub_rn(__dadd_rn(a, b), t);
}

__global__ void __launch_bounds__(256) k_tree_find(GrowBuf B, int d, int f0, int nf, int first) {
  __shared__ long long sG[TREE_BINS];
  __shared__ int sH[TREE_BINS];
  __shared__ double sg[TREE_BINS];
  __shared__ int sb[TREE_BINS];
  const int tid = threadIdx.x, nn = 1 << d, pos = blockIdx.x, c = blockIdx.y;
  if (B.state[c * B.NN + nn - 1 + pos] != 1) return;
  TreeRec* out = B.rec + (c * (1 << (B.depth - 1)) + pos);
  TreeRec best;
  if (first) { best.gain = -INFINITY; best.GL = 0; best.G = 0; best.HL = 0; best.H = 0; best.feat = -1; best.bin = 0; }
  else best = *out;
  const double sc = ldexp(1.0, -B.shift[c]);
  for (int fi = 0; fi < nf; ++fi) {
    const int f = B.flist[f0 + fi];
    const int nb = B.ncuts[f] + 1;
    const int64_t hb = (int64_t(c * nn + pos) * B.FT + fi) * TREE_BINS;
    __syncthreads();
    sG[tid] = B.histG[hb + tid];
    sH[tid] = B.histH[hb + tid];
    __syncthreads();
    for (int off = 1; off < TREE_BINS; off <<= 1) {
      const long long tg = tid >= off ? sG[tid - off] : 0;
      const int th = tid >= off ? sH[tid - off] : 0;
      __syncthreads();
      sG[tid] += tg;
      sH[tid] += th;
      __syncthreads();
    }
    const long long GL = sG[tid], G = sG[TREE_BINS - 1];
    const int HL = sH[tid], H = sH[TREE_BINS - 1];
    double gain = -INFINITY;
    if (tid < nb - 1 && double(HL) >= B.mcw && double(H - HL) >= B.mcw) gain = tree_gain(GL, HL, G, H, sc);
    sg[tid] = gain;
    sb[tid] = tid;
    __syncthreads();
    for (int s = TREE_BINS / 2; s > 0; s >>= 1) {
      if (tid < s) {
        const double o = sg[tid + s];
        if (o > sg[tid] || (o == sg[tid] && sb[tid + s] < sb[tid])) { sg[tid] = o; sb[tid] = sb[tid + s]; }
      }
      __syncthreads();
    }
    if (tid == 0) {
      best.G = G; best.H = H;
      if (sg[0] > best.gain) { best.gain = sg[0]; best.feat = f; best.bin = sb[0]; best.GL = sG[sb[0]]; best.HL = sH[sb[0]]; }
    }
  }
  if (tid == 0) *out = best;
}

__global__ void __launch_bounds__(256) k_tree_commit(GrowBuf B, int d) {
  const int nn = 1 << d, e = blockIdx.x * 256 + threadIdx.x;
  if (e >= B.k * nn) return;
  const int c = e / nn, pos = e % nn, node = nn - 1 + pos, at = c * B.NN + node;
  if (B.state[at] != 1) return;
  const TreeRec r = B.rec[c * (1 << (B.depth - 1)) + pos];
  B.nodeG[at] = r.G;
  B.nodeH[at] = r.H;
  if (r.gain > 0.0) {
    B.state[at] = 2;
    B.feat[at] = r.feat; B.bin[at] = r.bin; B.gain[at] = r.gain;
    B.thr[at] = B.cuts[int64_t(r.feat) * TREE_BINS + r.bin];
    const int l = c * B.NN + 2 * node + 1;
    B.state[l] = 1; B.nodeG[l] = r.GL; B.nodeH[l] = r.HL;
    B.state[l + 1] = 1; B.nodeG[l + 1] = r.G - r.GL; B.nodeH[l + 1] = r.H - r.HL;
  }
}

__global__ void __launch_bounds__(256) k_tree_part(GrowBuf B, int d) {
  const int nn = 1 << d;
  for (int64_t r = int64_t(blockIdx.x) * 256 + threadIdx.x; r < B.n; r += int64_t(gridDim.x) * 256) {
    for (int c = 0; c < B.k; ++c) {
      const int pos = B.nid[int64_t(c) * B.n + r];
      int right = 0;
      if (pos < nn) {
        const int at = c * B.NN + nn - 1 + pos;
        if (B.state[at] == 2) right = B.bins[int64_t(B.feat[at]) * B.n + r] > B.bin[at] ? 1 : 0;
      }
      B.nid[int64_t(c) * B.n + r] = uint8_t(2 * pos + right);
    }
  }
}

__global__ void __launch_bounds__(256) k_tree_leaf(GrowBuf B) {
#pragma clang fp contract(off)
  const int D = B.depth, nl = 1 << D, e = blockIdx.x * 256 + threadIdx.x;
  if (e >= B.k * nl) return;
  const int c = e / nl, j = e % nl;
  const double sc = ldexp(1.0, -B.shift[c]);
  float val = 0.0f;
  for (int d = 0; d <= D; ++d) {
    const int node = (1 << d) - 1 + (j >> (D - d)), at = c * B.NN + node;
    const int st = B.state[at];
    if (st == 2) continue;
    if (st == 1) {
      val = float(__ddiv_rn(__dmul_rn(-B.lr, __dmul_rn(double(B.nodeG[at]), sc)), __dadd_rn(double(B.nodeH[at]), 1.0)));
      if ((j & ((1 << (D - d)) - 1)) == 0) B.leaf[at] = val;
    }
    break;
  }
  B.leaftab[e] = val;
}

// T (n x k, float32) += the leaf under every row
__global__ void __launch_bounds__(256) k_tree_update(GrowBuf B, float* __restrict__ T) {
  const int nl = 1 << B.depth;
  const int64_t total = B.n * B.k;
  for (int64_t e = int64_t(blockIdx.x) * 256 + threadIdx.x; e < total; e += int64_t(gridDim.x) * 256) {
    const int64_t r = e / B.k;
    const int c = int(e % B.k);
    T[e] = T[e] + B.leaftab[c * nl + B.nid[int64_t(c) * B.n + r]];
  }
}

unsigned grid_for(int64_t items, int64_t most = 4096) { return unsigned(std::max<int64_t>(1, std::min<int64_t>((items + 255) / 256, most))); }

int feature_tile(int k, int depth, int nsel, size_t cap) {
  const size_t per = size_t(k) * (size_t(1) << (depth - 1)) * TREE_BINS * 12;
  return int(std::max<size_t>(1, std::min<size_t>(size_t(nsel), cap / per)));
}

// the k trees of one view: B.feat .. B.leaf, B.nid and B.leaftab on return (enqueued; no host wait)
void enqueue_grow(ccz_ctx* c, const GrowBuf& B) {
  hipStream_t st = stream(c);
  hipLaunchKernelGGL(k_tree_grow_init, dim3(grid_for(int64_t(B.k) * B.n)), dim3(256), 0, st, B);
  CCZ_LAUNCH_CHECK();
  const unsigned nchunk = unsigned((B.n + TREE_HROWS - 1) / TREE_HROWS);
  for (int d = 0; d < B.depth; ++d) {
    const int nn = 1 << d;
    const int lds = B.k * nn * TREE_BINS <= TREE_LDS_ENT ? 1 : 0;
    const size_t ent = size_t(B.k) * nn * B.FT * TREE_BINS;
    for (int f0 = 0; f0 < B.nsel; f0 += B.FT) {
      const int nf = std::min(B.FT, B.nsel - f0);
      CCZ_HIP(hipMemsetAsync(B.histG, 0, ent * 8, st));
      CCZ_HIP(hipMemsetAsync(B.histH, 0, ent * 4, st));
      hipLaunchKernelGGL(k_tree_hist, dim3(nchunk, unsigned(nf)), dim3(256), 0, st, B, d, f0, lds);
      CCZ_LAUNCH_CHECK();
      hipLaunchKernelGGL(k_tree_find, dim3(unsigned(nn), unsigned(B.k)), dim3(256), 0, st, B, d, f0, nf, f0 == 0 ? 1 : 0);
      CCZ_LAUNCH_CHECK();
    }
    hipLaunchKernelGGL(k_tree_commit, dim3(grid_for(int64_t(B.k) * nn)), dim3(256), 0, st, B, d);
    CCZ_LAUNCH_CHECK();
    hipLaunchKernelGGL(k_tree_part, dim3(grid_for(B.n)), dim3(256), 0, st, B, d);
    CCZ_LAUNCH_CHECK();
  }
  hipLaunchKernelGGL(k_tree_leaf, dim3(grid_for(int64_t(B.k) << B.depth)), dim3(256), 0, st, B);
  CCZ_LAUNCH_CHECK();
}

// ---- setup: cuts, bins, base margin ----------------------------------------------------------------------------------------
template <typename T>
__device__ __forceinline__ float centred32(const T* __restrict__ X, int64_t ld, const T* __restrict__ mu, int64_t r, int f) {
  const T d = mu ? T(X[r * ld + f] - mu[f]) : X[r * ld + f];
  return float(d);
}

template <typename T>
__global__ void __launch_bounds__(256) k_tree_cuts(const T* __restrict__ X, int64_t ld, const T* __restrict__ mu,
                                                   const long long* __restrict__ rows, int S, int64_t n, float* __restrict__ cuts,
                                                   int* __restrict__ ncuts) {
  __shared__ float s[TREE_CUT_SAMPLE];
  __shared__ unsigned char keep[TREE_BINS];
  const int tid = threadIdx.x, f = blockIdx.x;
  int N = 1;
  while (N < S) N <<= 1;
  for (int i = tid; i < N; i += 256) {
    float v = INFINITY;
    if (i < S) {
      const long long r = rows[i];
      if (r >= 0 && r < n) v = centred32(X, ld, mu, r, f);
    }
    s[i] = v;
  }
  __syncthreads();
  for (int k2 = 2; k2 <= N; k2 <<= 1) {
    for (int j = k2 >> 1; j > 0; j >>= 1) {
      for (int i = tid; i < N; i += 256) {
        const int x = i ^ j;
        if (x > i) {
          const bool up = (i & k2) == 0;
          const float a = s[i], b = s[x];
          if ((a > b) == up) { s[i] = b; s[x] = a; }
        }
      }
      __syncthreads();
    }
  }
  if (tid >= 1) {
    const float v = s[(tid * S) / TREE_BINS];
    const float prev = tid == 1 ? s[0] : s[((tid - 1) * S) / TREE_BINS];
    keep[tid] = v != prev ? 1 : 0;
  }
  __syncthreads();
  if (tid == 0) {
    int cnt = 0;
    for (int j = 1; j < TREE_BINS; ++j)
      if (keep[j]) cuts[int64_t(f) * TREE_BINS + cnt++] = s[(j * S) / TREE_BINS];
    ncuts[f] = cnt;
    for (int j = cnt; j < TREE_BINS; ++j) cuts[int64_t(f) * TREE_BINS + j] = INFINITY;
  }
}

template <typename T>
__global__ void __launch_bounds__(256) k_tree_bin(const T* __restrict__ X, int64_t ld, const T* __restrict__ mu, int64_t n,
                                                  const float* __restrict__ cuts, const int* __restrict__ ncuts,
                                                  uint8_t* __restrict__ bins) {
  const int f = blockIdx.y;
  const int64_t r = int64_t(blockIdx.x) * 256 + threadIdx.x;
  if (r >= n) return;
  const float x = centred32(X, ld, mu, r, f);
  const float* cf = cuts + int64_t(f) * TREE_BINS;
  int lo = 0, hi = ncuts[f];                    // the number of cuts <= x
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (cf[mid] <= x) lo = mid + 1; else hi = mid;
  }
  bins[int64_t(f) * n + r] = uint8_t(lo);
}

// out (n x k, float64) = (X - mu) W, the centred entries as the view's dtype holds them; W p x k float64
template <typename T>
__global__ void __launch_bounds__(256) k_tree_project(const T* __restrict__ X, int64_t ld, const T* __restrict__ mu, int64_t n, int p,
                                                      int k, const double* __restrict__ W, double* __restrict__ out, int64_t ldo) {
  const int64_t total = n * k;
  for (int64_t e = int64_t(blockIdx.x) * 256 + threadIdx.x; e < total; e += int64_t(gridDim.x) * 256) {
    const int64_t r = e / k;
    const int c = int(e % k);
    double s = 0.0;
    if (W)
      for (int f = 0; f < p; ++f) {
        const T d = mu ? T(X[r * ld + f] - mu[f]) : X[r * ld + f];
        s += double(d) * W[int64_t(f) * k + c];
      }
    out[r * ldo + c] = s;
  }
}

// grid k: the sum of squares of column blockIdx.x of Z (n x k)
__global__ void __launch_bounds__(256) k_tree_colsumsq(const double* __restrict__ Z, int64_t n, int k, double* __restrict__ out) {
  __shared__ double red[4];
  double s = 0.0;
  for (int64_t r = threadIdx.x; r < n; r += 256) { const double z = Z[r * k + blockIdx.x]; s += z * z; }
  s = block_sum<4>(s, red);
  if (threadIdx.x == 0) out[blockIdx.x] = s;
}

__global__ void __launch_bounds__(256) k_tree_margin(const double* __restrict__ Z, const double* __restrict__ scale, int64_t n, int k,
                                                     float* __restrict__ bm, float* __restrict__ T) {
  const int64_t total = n * k;
  for (int64_t e = int64_t(blockIdx.x) * 256 + threadIdx.x; e < total; e += int64_t(gridDim.x) * 256) {
    bm[e] = float(Z[e] / scale[e % k]);
    T[e] = 0.0f;
  }
}

__global__ void __launch_bounds__(256) k_tree_mask(uint64_t stream_key, uint64_t thr, int all, int64_t n, uint8_t* __restrict__ mask) {
  for (int64_t r = int64_t(blockIdx.x) * 256 + threadIdx.x; r < n; r += int64_t(gridDim.x) * 256)
    mask[r] = (all || splitmix64(stream_key ^ splitmix64(uint64_t(r))) < thr) ? 1 : 0;
}

// ---- the gradient ----------------------------------------------------------------------------------------------------------
struct ZViews {
  const float* bm[TREE_MAXVIEWS];
  const float* T[TREE_MAXVIEWS];
};
struct GStat {
  double scale;
  int shift[TREE_MAXVIEWS * TREE_MAXK];
};

__device__ __forceinline__ double zval(const ZViews& Z, int v, int64_t e) { return double(Z.bm[v][e]) + double(Z.T[v][e]); }

// grid (row chunks): part[(chunk M + v) (k k + k) + e] = sum over the chunk's rows of z_a z_b (e = a k + b) or z_a (e = k k + a)
__global__ void __launch_bounds__(256) k_tree_zmom(ZViews Z, int M, int64_t n, int k, int rc, double* __restrict__ part) {
  __shared__ double zs[64 * TREE_MAXK];
  const int tid = threadIdx.x, kk = k * k, ne = kk + k;
  const int64_t rb = int64_t(blockIdx.x) * rc, re = min(n, rb + rc);
  for (int v = 0; v < M; ++v) {
    double acc[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
    for (int64_t t0 = rb; t0 < re; t0 += 64) {
      const int rows = int(min(int64_t(64), re - t0));
      __syncthreads();
      for (int e = tid; e < rows * k; e += 256) zs[e] = zval(Z, v, t0 * k + e);
      __syncthreads();
#pragma unroll
      for (int i = 0; i < 5; ++i) {
        const int e = tid + 256 * i;
        if (e >= ne) break;
        double s = acc[i];
        if (e < kk) {
          const int a = e / k, b = e % k;
          for (int r = 0; r < rows; ++r) s += zs[r * k + a] * zs[r * k + b];
        } else {
          const int a = e - kk;
          for (int r = 0; r < rows; ++r) s += zs[r * k + a];
        }
        acc[i] = s;
      }
    }
#pragma unroll
    for (int i = 0; i < 5; ++i) {
      const int e = tid + 256 * i;
      if (e < ne) part[(int64_t(blockIdx.x) * M + v) * ne + e] = acc[i];
    }
  }
}

// one workgroup: the chunks folded in index order into mom (M (k k + k)), then mean (M k) and V (k k), the mean auto-covariance
__global__ void __launch_bounds__(256) k_tree_zfold(const double* __restrict__ part, int nchunk, int M, int64_t n, int k,
                                                    double* __restrict__ mom, double* __restrict__ mean, double* __restrict__ V) {
  const int tid = threadIdx.x, kk = k * k, ne = kk + k;
  for (int e = tid; e < M * ne; e += 256) {
    double s = 0.0;
    for (int g = 0; g < nchunk; ++g) s += part[int64_t(g) * M * ne + e];
    mom[e] = s;
  }
  __threadfence_block();
  __syncthreads();
  for (int e = tid; e < M * k; e += 256) mean[e] = mom[(e / k) * ne + kk + e % k] / double(n);
  for (int e = tid; e < kk; e += 256) {
    const int a = e / k, b = e % k;
    double s = 0.0;
    for (int v = 0; v < M; ++v) {
      const double* mv = mom + v * ne;
      s += (mv[e] - mv[kk + a] * mv[kk + b] / double(n)) / double(n - 1);
    }
    V[e] = s / double(M);
  }
}

// g (M x n x k) = scale (Zc_v V - sum_u Zc_u); gpart[(blk M + v) (2 + k)]: sum g, sum g^2, max |g| per column of this workgroup's rows
__global__ void __launch_bounds__(256) k_tree_grad(ZViews Z, int M, int64_t n, int k, double scale, const double* __restrict__ mean,
                                                   const double* __restrict__ V, double* __restrict__ g, double* __restrict__ gpart) {
  __shared__ double Vs[TREE_MAXK * TREE_MAXK];
  __shared__ double ms[TREE_MAXVIEWS * TREE_MAXK];
  __shared__ unsigned long long mx[TREE_MAXK];
  __shared__ double red[4];
  const int tid = threadIdx.x;
  for (int e = tid; e < k * k; e += 256) Vs[e] = V[e];
  for (int e = tid; e < M * k; e += 256) ms[e] = mean[e];
  __syncthreads();
  const int64_t total = n * k, e = int64_t(blockIdx.x) * 256 + tid;
  const bool on = e < total;
  const int64_t r = on ? e / k : 0;
  const int c = on ? int(e % k) : 0;
  double tot = 0.0;
  if (on)
    for (int u = 0; u < M; ++u) tot += zval(Z, u, e) - ms[u * k + c];
  for (int v = 0; v < M; ++v) {
    double gv = 0.0;
    if (on) {
      double s = 0.0;
      for (int a = 0; a < k; ++a) s += (zval(Z, v, r * k + a) - ms[v * k + a]) * Vs[a * k + c];
      gv = scale * (s - tot);
      g[int64_t(v) * total + e] = gv;
    }
    if (tid < k) mx[tid] = 0ull;
    __syncthreads();
    if (on) atomicMax(&mx[c], static_cast<unsigned long long>(__double_as_longlong(fabs(gv))));
    const double s1 = block_sum<4>(gv, red);
    const double s2 = block_sum<4>(gv * gv, red);
    __syncthreads();
    double* gp = gpart + (int64_t(blockIdx.x) * M + v) * (2 + k);
    if (tid == 0) { gp[0] = s1; gp[1] = s2; }
    if (tid < k) gp[2 + tid] = __longlong_as_double(static_cast<long long>(mx[tid]));
    __syncthreads();
  }
}

__global__ void __launch_bounds__(256) k_tree_gfin(const double* __restrict__ gpart, int nblk, int M, int64_t n, int k, GStat* st) {
  __shared__ double red[4];
  __shared__ double sd[TREE_MAXVIEWS];
  const int tid = threadIdx.x, w = 2 + k;
  const double N = double(n) * double(k);
  for (int v = 0; v < M; ++v) {
    double s1 = 0.0, s2 = 0.0;
    for (int g = tid; g < nblk; g += 256) { s1 += gpart[(int64_t(g) * M + v) * w]; s2 += gpart[(int64_t(g) * M + v) * w + 1]; }
    s1 = block_sum<4>(s1, red);
    s2 = block_sum<4>(s2, red);
    if (tid == 0) { const double m = s1 / N; sd[v] = sqrt(fmax(s2 / N - m * m, 0.0)); }
  }
  __syncthreads();
  double scale = 1e-6;
  for (int v = 0; v < M; ++v) scale = fmax(scale, sd[v]);
  if (tid == 0) st->scale = scale;
  for (int e = tid; e < M * k; e += 256) {
    const int v = e / k, c = e % k;
    double m = 0.0;
    for (int g = 0; g < nblk; ++g) m = fmax(m, gpart[(int64_t(g) * M + v) * w + 2 + c]);
    const float m32 = float(m / scale * TREE_TARGET_STD);
    st->shift[v * TREE_MAXK + c] = m32 > 0.0f ? 29 - ilogbf(m32) : 0;
  }
}

// q (k x n) = rint(float(g / scale * 0.1) 2^S) of view v; sh (k ints) = its shifts
__global__ void __launch_bounds__(256) k_tree_quant(const double* __restrict__ g, const GStat* __restrict__ st, int v, int64_t n, int k,
                                                    int* __restrict__ q, int* __restrict__ sh) {
  const int64_t total = n * k;
  const double scale = st->scale;
  for (int64_t e = int64_t(blockIdx.x) * 256 + threadIdx.x; e < total; e += int64_t(gridDim.x) * 256) {
    const int64_t r = e / k;
    const int c = int(e % k);
    const float g32 = float(g[e] / scale * TREE_TARGET_STD);
    q[int64_t(c) * n + r] = int(rint(ldexp(double(g32), st->shift[v * TREE_MAXK + c])));
  }
  if (blockIdx.x == 0 && threadIdx.x < k) sh[threadIdx.x] = st->shift[v * TREE_MAXK + threadIdx.x];
}

__global__ void __launch_bounds__(256) k_tree_embed(ZViews Z, int v, int64_t total, double* __restrict__ out) {
  for (int64_t e = int64_t(blockIdx.x) * 256 + threadIdx.x; e < total; e += int64_t(gridDim.x) * 256) out[e] = zval(Z, v, e);
}

struct TreeStatus {
  long long rounds;
  int stopped;
};
__global__ void k_tree_round_done(TreeStatus* st, long long total) {
  st->rounds += 1;
  if (st->rounds >= total) st->stopped = 1;
}
__global__ void k_tree_status0(TreeStatus* st) { st->rounds = 0; st->stopped = 0; }

// ---- predict ---------------------------------------------------------------------------------------------------------------
// out (n x k, float64) = (X - mu) P + double(sum of the float32 leaves in tree order); trees [ntrees][k][NN]
template <typename T>
__global__ void __launch_bounds__(256) k_tree_predict(const T* __restrict__ X, int64_t ld, const T* __restrict__ mu, int64_t n, int p,
                                                      int k, const double* __restrict__ P, int ntrees, int depth,
                                                      const int* __restrict__ feat, const float* __restrict__ thr,
                                                      const float* __restrict__ leaf, double* __restrict__ out, int64_t ldo) {
  const int NN = (2 << depth) - 1;
  const int64_t total = n * k;
  for (int64_t e = int64_t(blockIdx.x) * 256 + threadIdx.x; e < total; e += int64_t(gridDim.x) * 256) {
    const int64_t r = e / k;
    const int c = int(e % k);
    double bmv = 0.0;
    if (P)
      for (int f = 0; f < p; ++f) {
        const T d = mu ? T(X[r * ld + f] - mu[f]) : X[r * ld + f];
        bmv += double(d) * P[int64_t(f) * k + c];
      }
    float s = 0.0f;
    for (int t = 0; t < ntrees; ++t) {
      const int64_t tb = (int64_t(t) * k + c) * NN;
      int node = 0;
      for (int d = 0; d < depth; ++d) {
        const int f = feat[tb + node];
        if (f < 0 || f >= p) break;
        node = 2 * node + 1 + (centred32(X, ld, mu, r, f) < thr[tb + node] ? 0 : 1);
      }
      s = s + leaf[tb + node];
    }
    out[r * ldo + c] = bmv + double(s);
  }
}

// ---- the fit state ---------------------------------------------------------------------------------------------------------
struct TreeView {
  int p = 0, nsel = 0;
  uint8_t* bins = nullptr;
  float* cuts = nullptr;
  int* ncuts = nullptr;
  float* bm = nullptr;
  float* T = nullptr;
  int* flist = nullptr;            // rounds x nsel
  int* feat = nullptr; int* bin = nullptr; float* thr = nullptr; float* leaf = nullptr; double* gain = nullptr;   // rounds x k x NN
};

struct TreeState : FitState<TreeStatus> {
  int64_t n = 0;
  int k = 0, depth = 0, NN = 0, rounds = 0, gs = 0, nchunk = 0, rc = 0, gblk = 0;
  int64_t enq = 0;                 // rounds enqueued
  double lr = 0.0, mcw = 0.0;
  uint64_t seed = 0, thr = 0;
  int all_rows = 0;
  std::vector<TreeView> vw;
  ZViews Z;
  double* g = nullptr;             // M x n x k
  double* zpart = nullptr; double* mom = nullptr; double* mean = nullptr; double* V = nullptr; double* gpart = nullptr;
  GStat* gstat = nullptr;
  int* q = nullptr; int* shift = nullptr;
  uint8_t* nid = nullptr; uint8_t* mask = nullptr;
  long long* histG = nullptr; int* histH = nullptr;
  TreeRec* rec = nullptr;
  long long* nodeG = nullptr; int* nodeH = nullptr; uint8_t* state = nullptr;
  float* leaftab = nullptr;
  bool binned = false, margin = false, features = false;
};

uint64_t stream_key(uint64_t seed, uint64_t tag) { return splitmix64(seed ^ splitmix64(tag)); }

void enqueue_gradient(ccz_ctx* c, TreeState& S) {
  hipStream_t st = stream(c);
  hipLaunchKernelGGL(k_tree_zmom, dim3(unsigned(S.nchunk)), dim3(256), 0, st, S.Z, S.M, S.n, S.k, S.rc, S.zpart);
  CCZ_LAUNCH_CHECK();
  hipLaunchKernelGGL(k_tree_zfold, dim3(1), dim3(256), 0, st, S.zpart, S.nchunk, S.M, S.n, S.k, S.mom, S.mean, S.V);
  CCZ_LAUNCH_CHECK();
  hipLaunchKernelGGL(k_tree_grad, dim3(unsigned(S.gblk)), dim3(256), 0, st, S.Z, S.M, S.n, S.k, 4.0 / (double(S.M) * double(S.n - 1)),
                     S.mean, S.V, S.g, S.gpart);
  CCZ_LAUNCH_CHECK();
  hipLaunchKernelGGL(k_tree_gfin, dim3(1), dim3(256), 0, st, S.gpart, S.gblk, S.M, S.n, S.k, S.gstat);
  CCZ_LAUNCH_CHECK();
}

GrowBuf grow_buf(const TreeState& S, int v, int64_t round) {
  const TreeView& W = S.vw[v];
  GrowBuf B;
  memset(&B, 0, sizeof(B));
  B.bins = W.bins; B.cuts = W.cuts; B.ncuts = W.ncuts; B.q = S.q; B.mask = S.mask; B.flist = W.flist + round * W.nsel;
  B.shift = S.shift; B.nid = S.nid; B.histG = S.histG; B.histH = S.histH; B.rec = S.rec; B.nodeG = S.nodeG; B.nodeH = S.nodeH;
  B.state = S.state; B.leaftab = S.leaftab;
  const int64_t off = round * S.k * S.NN;
  B.feat = W.feat + off; B.bin = W.bin + off; B.thr = W.thr + off; B.leaf = W.leaf + off; B.gain = W.gain + off;
  B.n = S.n; B.p = W.p; B.k = S.k; B.depth = S.depth; B.nsel = W.nsel; B.NN = S.NN;
  B.FT = feature_tile(S.k, S.depth, W.nsel, TREE_HIST_BYTES);
  B.lr = S.lr; B.mcw = S.mcw;
  return B;
}

void enqueue_round(ccz_ctx* c, TreeState& S) {
  hipStream_t st = stream(c);
  const int64_t t = S.enq;
  hipLaunchKernelGGL(k_tree_mask, dim3(grid_for(S.n)), dim3(256), 0, st, stream_key(S.seed, uint64_t(2 * t)), S.thr, S.all_rows, S.n, S.mask);
  CCZ_LAUNCH_CHECK();
  enqueue_gradient(c, S);
  for (int v = 0; v < S.M; ++v) {
    hipLaunchKernelGGL(k_tree_quant, dim3(grid_for(S.n * S.k)), dim3(256), 0, st, S.g + int64_t(v) * S.n * S.k, S.gstat, v, S.n, S.k, S.q,
                       S.shift);
    CCZ_LAUNCH_CHECK();
    const GrowBuf B = grow_buf(S, v, t);
    enqueue_grow(c, B);
    hipLaunchKernelGGL(k_tree_update, dim3(grid_for(S.n * S.k)), dim3(256), 0, st, B, S.vw[v].T);
    CCZ_LAUNCH_CHECK();
    if (S.gs && v < S.M - 1) enqueue_gradient(c, S);
  }
  hipLaunchKernelGGL(k_tree_round_done, dim3(1), dim3(1), 0, st, S.drv.dev, (long long)S.rounds);
  CCZ_LAUNCH_CHECK();
  S.enq = t + 1;
}

void check_shape(int64_t n, int64_t p, int64_t k, int64_t depth) {
  if (n < 1 || n > TREE_MAXN) fail(CCZ_EUNSUP, "tree: 1 to %lld rows are supported, got %lld", (long long)TREE_MAXN, (long long)n);
  if (p < 1 || p > TREE_MAXP) fail(CCZ_EUNSUP, "tree: 1 to %lld features per view are supported, got %lld", (long long)TREE_MAXP, (long long)p);
  if (k < 1 || k > TREE_MAXK) fail(CCZ_EUNSUP, "tree: 1 to %d components are supported, got %lld", TREE_MAXK, (long long)k);
  if (depth < 1 || depth > TREE_MAXDEPTH) fail(CCZ_EUNSUP, "tree: max_depth must be 1..%d, got %lld", TREE_MAXDEPTH, (long long)depth);
}

void check_flist(const int* fl, int64_t count, int nsel, int p) {
  for (int64_t i = 0; i < count; ++i) {
    if (fl[i] < 0 || fl[i] >= p) fail(CCZ_EINVAL, "tree: feature index %d out of range", fl[i]);
    if (i % nsel && fl[i] <= fl[i - 1]) fail(CCZ_EINVAL, "tree: a feature list must ascend");
  }
}

TreeState* tree_create(ccz_ctx* c, int M, const int64_t* p, int64_t n, int64_t k, int64_t depth, int64_t rounds, double lr, double mcw,
                       int gs, double subsample, uint64_t seed, int64_t chunk) {
  check_view_count("tree", M, TREE_MAXVIEWS);
  if (!p) fail(CCZ_EINVAL, "tree: null argument");
  if (M < 2) fail(CCZ_EINVAL, "tree: at least 2 views");
  for (int i = 0; i < M; ++i) check_shape(n, p[i], k, depth);
  if (n < 2) fail(CCZ_EINVAL, "tree: at least 2 rows");
  if (rounds < 1 || rounds > 100000 || chunk < 1 || !(lr > 0.0) || !(mcw >= 0.0) || !(subsample > 0.0) || !(subsample <= 1.0))
    fail(CCZ_EINVAL, "tree: bad argument");
  for (int i = 0; i < M; ++i)
    if (k > p[i]) fail(CCZ_EINVAL, "tree: %lld components exceed the %lld features of view %d", (long long)k, (long long)p[i], i);
  return new_state<TreeState>(c, [&](TreeState& S) {
    S.dtype = CCZ_F64; S.M = M; S.chunk = chunk;
    S.p.assign(p, p + M);
    S.n = n; S.k = int(k); S.depth = int(depth); S.NN = (2 << depth) - 1; S.rounds = int(rounds); S.gs = gs; S.lr = lr; S.mcw = mcw;
    S.seed = seed;
    S.all_rows = subsample >= 1.0 ? 1 : 0;
    S.thr = S.all_rows ? ~uint64_t(0) : uint64_t(ldexp(subsample, 64));
    row_chunks(n, 256, &S.nchunk, &S.rc);
    S.gblk = int((n * k + 255) / 256);
    const size_t nk = size_t(n) * size_t(k), ne = size_t(k) * k + k, tn = size_t(rounds) * k * S.NN;
    memset(&S.Z, 0, sizeof(S.Z));
    S.vw.resize(M);
    for (int i = 0; i < M; ++i) {
      TreeView& W = S.vw[i];
      W.p = int(p[i]);
      W.bins = S.get<uint8_t>(c, size_t(p[i]) * n);
      W.cuts = S.get<float>(c, size_t(p[i]) * TREE_BINS);
      W.ncuts = S.get<int>(c, size_t(p[i]));
      W.bm = S.get<float>(c, nk);
      W.T = S.get<float>(c, nk);
      W.feat = S.get<int>(c, tn); W.bin = S.get<int>(c, tn); W.thr = S.get<float>(c, tn); W.leaf = S.get<float>(c, tn);
      W.gain = S.get<double>(c, tn);
      S.Z.bm[i] = W.bm; S.Z.T[i] = W.T;
    }
    S.g = S.get(c, size_t(M) * nk);
    S.zpart = S.get(c, size_t(S.nchunk) * M * ne);
    S.mom = S.get(c, size_t(M) * ne); S.mean = S.get(c, size_t(M) * k); S.V = S.get(c, size_t(k) * k);
    S.gpart = S.get(c, size_t(S.gblk) * M * (2 + k));
    S.gstat = S.get<GStat>(c, 1);
    S.q = S.get<int>(c, nk); S.shift = S.get<int>(c, size_t(k));
    S.nid = S.get<uint8_t>(c, nk); S.mask = S.get<uint8_t>(c, size_t(n));
    const size_t hist = size_t(k) * (size_t(1) << (depth - 1)) * TREE_BINS *
                        size_t(feature_tile(int(k), int(depth), int(*std::max_element(p, p + M)), TREE_HIST_BYTES));
    S.histG = S.get<long long>(c, hist); S.histH = S.get<int>(c, hist);
    S.rec = S.get<TreeRec>(c, size_t(k) << (depth - 1));
    S.nodeG = S.get<long long>(c, size_t(k) * S.NN); S.nodeH = S.get<int>(c, size_t(k) * S.NN); S.state = S.get<uint8_t>(c, size_t(k) * S.NN);
    S.leaftab = S.get<float>(c, size_t(k) << depth);
    S.drv.create(c);
  });
}

template <typename T>
void enqueue_bins(ccz_ctx* c, const T* X, int64_t ld, const T* mu, int64_t n, int p, const long long* rows, int S, float* cuts, int* ncuts,
                  uint8_t* bins) {
  hipLaunchKernelGGL((k_tree_cuts<T>), dim3(unsigned(p)), dim3(256), 0, stream(c), X, ld, mu, rows, S, n, cuts, ncuts);
  CCZ_LAUNCH_CHECK();
  hipLaunchKernelGGL((k_tree_bin<T>), dim3(unsigned((n + 255) / 256), unsigned(p)), dim3(256), 0, stream(c), X, ld, mu, n, cuts, ncuts, bins);
  CCZ_LAUNCH_CHECK();
}

struct Scratch {                   // device allocations of one call
  ccz_ctx* c;
  std::vector<void*> a;
  explicit Scratch(ccz_ctx* c_) : c(c_) {}
  ~Scratch() {
    for (void* p : a) dev_free(c, p);
  }
  template <typename T>
  T* get(size_t count) {
    a.push_back(dev_alloc(c, std::max<size_t>(count, 1) * sizeof(T)));
    return static_cast<T*>(a.back());
  }
  template <typename T>
  T* put(const T* host, size_t count) {
    T* d = get<T>(count);
    h2d(c, d, host, count * sizeof(T));
    return d;
  }
};

}  // namespace
}  // namespace ccz

extern "C" {

int ccz_tree_create(ccz_handle h, int n_views, const int64_t* p, int64_t n_rows, int64_t k, int64_t max_depth, int64_t n_rounds,
                    double learning_rate, double min_child_weight, int gauss_seidel, double subsample, uint64_t seed, int64_t chunk_rounds,
                    void** state_out) {
  CCZ_GUARD(h, {
    if (!state_out) ccz::fail(CCZ_EINVAL, "null argument");
    *state_out = nullptr;
    *state_out = ccz::tree_create(h, n_views, p, n_rows, k, max_depth, n_rounds, learning_rate, min_child_weight, gauss_seidel, subsample,
                                  seed, chunk_rounds);
  })
}

int ccz_tree_destroy(ccz_handle h, void* state) {
  CCZ_GUARD(h, {
    if (state) ccz::free_state(h, static_cast<ccz::TreeState*>(state));
  })
}

int ccz_tree_setup(ccz_handle h, void* state, int dtype, const ccz_view* views, const void* const* means_dev, const int64_t* sample_rows,
                   int64_t n_sample) {
  CCZ_GUARD(h, {
    ccz::TreeState& S = *ccz::as_state<ccz::TreeState>("tree", state);
    ccz::check_dtype("tree", dtype);
    if (!views || !sample_rows) ccz::fail(CCZ_EINVAL, "tree: null argument");
    if (n_sample != std::min<int64_t>(S.n, ccz::TREE_CUT_SAMPLE)) ccz::fail(CCZ_EINVAL, "tree: the cut sample must hold min(n, 8192) rows");
    for (int64_t i = 0; i < n_sample; ++i)
      if (sample_rows[i] < 0 || sample_rows[i] >= S.n) ccz::fail(CCZ_EINVAL, "tree: sample row out of range");
    for (int i = 0; i < S.M; ++i)
      if (!views[i].data || views[i].cols != S.p[i] || views[i].ld < views[i].cols) ccz::fail(CCZ_EINVAL, "tree: bad view %d", i);
    S.restart(h);
    S.binned = S.margin = false;
    ccz::Scratch tmp(h);
    const long long* rows = tmp.put(reinterpret_cast<const long long*>(sample_rows), size_t(n_sample));
    for (int i = 0; i < S.M; ++i) {
      ccz::TreeView& W = S.vw[i];
      ccz::by_dtype(dtype, [&](auto t) {
        using T = decltype(t);
        ccz::enqueue_bins<T>(h, static_cast<const T*>(views[i].data), views[i].ld, means_dev ? static_cast<const T*>(means_dev[i]) : nullptr,
                             S.n, W.p, rows, int(n_sample), W.cuts, W.ncuts, W.bins);
      });
    }
    ccz::sync(h);
    S.binned = true;
  })
}

int ccz_tree_project(ccz_handle h, void* state, int dtype, const ccz_view* views, const void* const* means_dev, const double* W_host,
                     double* sumsq_host) {
  CCZ_GUARD(h, {
    ccz::TreeState& S = *ccz::as_state<ccz::TreeState>("tree", state);
    ccz::check_dtype("tree", dtype);
    if (!views || !W_host || !sumsq_host) ccz::fail(CCZ_EINVAL, "tree: null argument");
    for (int i = 0; i < S.M; ++i)
      if (!views[i].data || views[i].cols != S.p[i] || views[i].ld < views[i].cols) ccz::fail(CCZ_EINVAL, "tree: bad view %d", i);
    S.margin = false;
    ccz::Scratch tmp(h);
    double* ss = tmp.get<double>(size_t(S.M) * S.k);
    const int64_t nk = S.n * S.k;
    int64_t off = 0;
    for (int i = 0; i < S.M; ++i) {
      const double* Wd = tmp.put(W_host + off, size_t(S.p[i]) * S.k);
      off += S.p[i] * S.k;
      double* Z0 = S.g + int64_t(i) * nk;
      ccz::by_dtype(dtype, [&](auto t) {
        using T = decltype(t);
        hipLaunchKernelGGL((ccz::k_tree_project<T>), dim3(ccz::grid_for(nk)), dim3(256), 0, ccz::stream(h), static_cast<const T*>(views[i].data),
                           views[i].ld, means_dev ? static_cast<const T*>(means_dev[i]) : nullptr, S.n, int(S.p[i]), S.k, Wd, Z0, int64_t(S.k));
      });
      CCZ_LAUNCH_CHECK();
      hipLaunchKernelGGL(ccz::k_tree_colsumsq, dim3(unsigned(S.k)), dim3(256), 0, ccz::stream(h), Z0, S.n, S.k, ss + i * S.k);
      CCZ_LAUNCH_CHECK();
    }
    ccz::d2h(h, sumsq_host, ss, size_t(S.M) * S.k * 8);
  })
}

int ccz_tree_set_margin(ccz_handle h, void* state, const double* scale_host) {
  CCZ_GUARD(h, {
    ccz::TreeState& S = *ccz::as_state<ccz::TreeState>("tree", state);
    if (!scale_host) ccz::fail(CCZ_EINVAL, "tree: null argument");
    for (int e = 0; e < S.M * S.k; ++e)
      if (!(scale_host[e] > 0.0) || !std::isfinite(scale_host[e])) ccz::fail(CCZ_EINVAL, "tree: a base-margin column has no variance");
    ccz::Scratch tmp(h);
    const double* sc = tmp.put(scale_host, size_t(S.M) * S.k);
    const int64_t nk = S.n * S.k;
    for (int i = 0; i < S.M; ++i) {
      hipLaunchKernelGGL(ccz::k_tree_margin, dim3(ccz::grid_for(nk)), dim3(256), 0, ccz::stream(h), S.g + int64_t(i) * nk, sc + i * S.k, S.n, S.k,
                         S.vw[i].bm, S.vw[i].T);
      CCZ_LAUNCH_CHECK();
    }
    hipLaunchKernelGGL(ccz::k_tree_status0, dim3(1), dim3(1), 0, ccz::stream(h), S.drv.dev);
    CCZ_LAUNCH_CHECK();
    ccz::sync(h);
    S.enq = 0;
    S.margin = true;
  })
}

int ccz_tree_set_features(ccz_handle h, void* state, const int* n_selected, const int* lists_host) {
  CCZ_GUARD(h, {
    ccz::TreeState& S = *ccz::as_state<ccz::TreeState>("tree", state);
    if (!n_selected || !lists_host) ccz::fail(CCZ_EINVAL, "tree: null argument");
    S.features = false;
    int64_t off = 0;
    for (int i = 0; i < S.M; ++i) {
      if (n_selected[i] < 1 || n_selected[i] > S.p[i]) ccz::fail(CCZ_EINVAL, "tree: view %d: 1 to %lld features per tree", i, (long long)S.p[i]);
      ccz::check_flist(lists_host + off, int64_t(S.rounds) * n_selected[i], n_selected[i], int(S.p[i]));
      off += int64_t(S.rounds) * n_selected[i];
    }
    ccz::sync(h);
    off = 0;
    for (int i = 0; i < S.M; ++i) {
      ccz::TreeView& W = S.vw[i];
      const size_t cnt = size_t(S.rounds) * n_selected[i];
      if (!W.flist || W.nsel != n_selected[i]) W.flist = S.get<int>(h, cnt);
      W.nsel = n_selected[i];
      ccz::h2d(h, W.flist, lists_host + off, cnt * sizeof(int));
      off += int64_t(cnt);
    }
    S.features = true;
  })
}

int ccz_tree_rounds(ccz_handle h, void* state, int64_t n_rounds, int64_t* rounds_known, int* stopped_known) {
  CCZ_GUARD(h, {
    ccz::TreeState& S = *ccz::as_state<ccz::TreeState>("tree", state);
    if (!S.binned || !S.margin || !S.features) ccz::fail(CCZ_EINVAL, "tree: setup, margin and features come first");
    if (n_rounds >= 0 && S.enq + n_rounds > S.rounds) ccz::fail(CCZ_EINVAL, "tree: more rounds than the fit state holds");
    ccz::run_chunk(h, "tree", "n_rounds", S, n_rounds, rounds_known, stopped_known, &ccz::TreeStatus::rounds, [] { return 0; },
                   [&](int, int64_t) { ccz::enqueue_round(h, S); });
  })
}

int ccz_tree_status(ccz_handle h, void* state, int64_t* rounds, int* stopped) {
  CCZ_GUARD(h, {
    ccz::TreeState& S = *ccz::as_state<ccz::TreeState>("tree", state);
    if (!S.margin) ccz::fail(CCZ_EINVAL, "tree: ccz_tree_set_margin has not been called");
    ccz::TreeStatus st;
    ccz::d2h(h, &st, S.drv.dev, sizeof(st));
    if (rounds) *rounds = st.rounds;
    if (stopped) *stopped = st.stopped;
  })
}

int ccz_tree_get_bins(ccz_handle h, void* state, int view, uint8_t* bins_host, float* cuts_host, int* ncuts_host) {
  CCZ_GUARD(h, {
    ccz::TreeState& S = *ccz::as_state<ccz::TreeState>("tree", state);
    if (!S.binned) ccz::fail(CCZ_EINVAL, "tree: ccz_tree_setup has not been called");
    if (view < 0 || view >= S.M) ccz::fail(CCZ_EINVAL, "tree: no view %d", view);
    const ccz::TreeView& W = S.vw[view];
    if (bins_host) ccz::d2h(h, bins_host, W.bins, size_t(W.p) * S.n);
    if (cuts_host) ccz::d2h(h, cuts_host, W.cuts, size_t(W.p) * ccz::TREE_BINS * 4);
    if (ncuts_host) ccz::d2h(h, ncuts_host, W.ncuts, size_t(W.p) * 4);
  })
}

int ccz_tree_get_trees(ccz_handle h, void* state, int view, int* feature_host, int* bin_host, float* threshold_host, float* leaf_host,
                       double* gain_host) {
  CCZ_GUARD(h, {
    ccz::TreeState& S = *ccz::as_state<ccz::TreeState>("tree", state);
    if (!S.margin) ccz::fail(CCZ_EINVAL, "tree: ccz_tree_set_margin has not been called");
    if (view < 0 || view >= S.M) ccz::fail(CCZ_EINVAL, "tree: no view %d", view);
    const ccz::TreeView& W = S.vw[view];
    const size_t tn = size_t(S.enq) * S.k * S.NN;
    if (tn == 0) return CCZ_OK;
    if (feature_host) ccz::d2h(h, feature_host, W.feat, tn * 4);
    if (bin_host) ccz::d2h(h, bin_host, W.bin, tn * 4);
    if (threshold_host) ccz::d2h(h, threshold_host, W.thr, tn * 4);
    if (leaf_host) ccz::d2h(h, leaf_host, W.leaf, tn * 4);
    if (gain_host) ccz::d2h(h, gain_host, W.gain, tn * 8);
  })
}

int ccz_tree_get_embedding(ccz_handle h, void* state, int view, double* Z_host, double* Z_dev) {
  CCZ_GUARD(h, {
    ccz::TreeState& S = *ccz::as_state<ccz::TreeState>("tree", state);
    if (!S.margin) ccz::fail(CCZ_EINVAL, "tree: ccz_tree_set_margin has not been called");
    if (view < 0 || view >= S.M) ccz::fail(CCZ_EINVAL, "tree: no view %d", view);
    const int64_t nk = S.n * S.k;
    double* out = S.g + int64_t(view) * nk;      // the gradient buffer is free between rounds
    hipLaunchKernelGGL(ccz::k_tree_embed, dim3(ccz::grid_for(nk)), dim3(256), 0, ccz::stream(h), S.Z, view, nk, out);
    CCZ_LAUNCH_CHECK();
    if (Z_dev) ccz::d2d(h, Z_dev, out, size_t(nk) * 8);
    if (Z_host) ccz::d2h(h, Z_host, out, size_t(nk) * 8);
  })
}

int ccz_tree_grow(ccz_handle h, int64_t n_rows, int64_t p, int64_t k, int64_t max_depth, const uint8_t* bins_host, const float* cuts_host,
                  const int* ncuts_host, const int* q_host, const int* shift_host, const uint8_t* mask_host, const int* features_host,
                  int64_t n_features, double learning_rate, double min_child_weight, int64_t hist_bytes, int* feature_out, int* bin_out,
                  float* threshold_out, float* leaf_out, double* gain_out, uint8_t* node_out) {
  CCZ_GUARD(h, {
    if (!bins_host || !cuts_host || !ncuts_host || !q_host || !shift_host || !mask_host || !features_host)
      ccz::fail(CCZ_EINVAL, "tree: null argument");
    ccz::check_shape(n_rows, p, k, max_depth);
    if (n_features < 1 || n_features > p) ccz::fail(CCZ_EINVAL, "tree: 1 to %lld features per tree", (long long)p);
    if (!(learning_rate > 0.0) || !(min_child_weight >= 0.0) || hist_bytes < 0) ccz::fail(CCZ_EINVAL, "tree: bad argument");
    ccz::check_flist(features_host, n_features, int(n_features), int(p));
    for (int64_t f = 0; f < p; ++f)
      if (ncuts_host[f] < 0 || ncuts_host[f] > ccz::TREE_BINS - 1) ccz::fail(CCZ_EINVAL, "tree: a feature has at most 255 cuts");
    for (int64_t c = 0; c < k; ++c)
      if (shift_host[c] < -1100 || shift_host[c] > 1100) ccz::fail(CCZ_EINVAL, "tree: bad shift");
    const int64_t n = n_rows;
    const int NN = (2 << max_depth) - 1;
    ccz::Scratch tmp(h);
    ccz::GrowBuf B;
    memset(&B, 0, sizeof(B));
    B.n = n; B.p = int(p); B.k = int(k); B.depth = int(max_depth); B.nsel = int(n_features); B.NN = NN;
    B.lr = learning_rate; B.mcw = min_child_weight;
    B.FT = ccz::feature_tile(B.k, B.depth, B.nsel, hist_bytes ? size_t(hist_bytes) : ccz::TREE_HIST_BYTES);
    B.bins = tmp.put(bins_host, size_t(p) * n);
    B.cuts = tmp.put(cuts_host, size_t(p) * ccz::TREE_BINS);
    B.ncuts = tmp.put(ncuts_host, size_t(p));
    B.q = tmp.put(q_host, size_t(k) * n);
    B.shift = tmp.put(shift_host, size_t(k));
    B.mask = tmp.put(mask_host, size_t(n));
    B.flist = tmp.put(features_host, size_t(n_features));
    const size_t kn = size_t(k) * NN, hist = size_t(k) * (size_t(1) << (max_depth - 1)) * B.FT * ccz::TREE_BINS;
    B.nid = tmp.get<uint8_t>(size_t(k) * n);
    B.histG = tmp.get<long long>(hist); B.histH = tmp.get<int>(hist);
    B.rec = tmp.get<ccz::TreeRec>(size_t(k) << (max_depth - 1));
    B.nodeG = tmp.get<long long>(kn); B.nodeH = tmp.get<int>(kn); B.state = tmp.get<uint8_t>(kn);
    B.feat = tmp.get<int>(kn); B.bin = tmp.get<int>(kn); B.thr = tmp.get<float>(kn); B.leaf = tmp.get<float>(kn); B.gain = tmp.get<double>(kn);
    B.leaftab = tmp.get<float>(size_t(k) << max_depth);
    ccz::enqueue_grow(h, B);
    if (feature_out) ccz::d2h(h, feature_out, B.feat, kn * 4);
    if (bin_out) ccz::d2h(h, bin_out, B.bin, kn * 4);
    if (threshold_out) ccz::d2h(h, threshold_out, B.thr, kn * 4);
    if (leaf_out) ccz::d2h(h, leaf_out, B.leaf, kn * 4);
    if (gain_out) ccz::d2h(h, gain_out, B.gain, kn * 8);
    if (node_out) ccz::d2h(h, node_out, B.nid, size_t(k) * n);
    ccz::sync(h);
  })
}

int ccz_tree_predict(ccz_handle h, int dtype, const ccz_view* view, int64_t n_rows, const void* mean_dev, const double* proj_dev, int64_t k,
                     int64_t n_trees, int64_t max_depth, const int* feature_dev, const float* threshold_dev, const float* leaf_dev,
                     double* out_dev, int64_t ldo) {
  CCZ_GUARD(h, {
    ccz::check_dtype("tree", dtype);
    if (!view || !view->data || !out_dev || view->ld < view->cols || ldo < k || n_trees < 0)
      ccz::fail(CCZ_EINVAL, "tree: bad argument");
    ccz::check_shape(n_rows, view->cols, k, max_depth);
    if (n_trees > 0 && (!feature_dev || !threshold_dev || !leaf_dev)) ccz::fail(CCZ_EINVAL, "tree: null trees");
    ccz::by_dtype(dtype, [&](auto t) {
      using T = decltype(t);
      hipLaunchKernelGGL((ccz::k_tree_predict<T>), dim3(ccz::grid_for(n_rows * k)), dim3(256), 0, ccz::stream(h),
                         static_cast<const T*>(view->data), view->ld, static_cast<const T*>(mean_dev), n_rows, int(view->cols), int(k), proj_dev,
                         int(n_trees), int(max_depth), feature_dev, threshold_dev, leaf_dev, out_dev, ldo);
    });
    CCZ_LAUNCH_CHECK();
  })
}

}  // extern "C"
