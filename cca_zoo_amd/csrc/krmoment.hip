// Khatri-Rao moment and its adjoint: the cross-moment tensor of V views and the contraction of a tensor with all views but one.
//
// Reference: cca_zoo/deep/objectives.py:279-288 (TCCALoss: the n x d_1 x .. x d_V outer-product tensor, then its mean over the
// batch), cca_zoo/linear/_tcca.py:99-109 (the same tensor of the whitened views).  Neither product ever forms the n x prod d
// tensor here: both are GEMMs whose left operand is a row-wise Khatri-Rao product that exists only in registers.
//
//   ccz_kr_moment   M (R x C) = scale A' H_V,   A[s, r] = prod_{i < V} H_i[s, r_i],  R = prod_{i < V} d_i,  C = d_V
//     k_kr_moment   grid (row tiles x column tiles, 1, sample splits), 256 threads.  A workgroup owns 64 tensor rows (16 per wave)
//                   x 64 columns.  v_mfma_f64_16x16x4f64: A operand row = lane & 15, sample = lane >> 4; B operand sample =
//                   lane >> 4, column = lane & 15; C/D column = lane & 15, row = (lane >> 4) + 4 reg.  A lane decomposes its row
//                   r -> (r_1 .. r_{V-1}) once; per chunk of 32 samples the workgroup stages, of every left view, only the WINDOW of
//                   columns its 64 rows touch (consecutive rows touch consecutive columns modulo d_i: at most 63 / stride_i + 2 of
//                   them), and 64 columns of H_V.  A lane's A value is then V - 1 LDS reads multiplied together.
//   ccz_kr_apply    out (n x d_j) = scale B_j T_(j),   B_j[s, r'] = prod_{i != j} H_i[s, r'_i],  r' over the other views' indices
//     k_kr_unfold   T -> T_(j) (mode j moved last; skipped when j is the last mode)
//     k_kr_apply    grid (sample tiles x column tiles, 1, reduction splits).  A workgroup owns 64 samples (16 per wave) x 64 columns;
//                   A operand row = sample, k = tensor row r'.  Per chunk of 32 tensor rows it stages the views' windows for its 64
//                   samples, 32 x 64 of T_(j), and a table of the chunk's window indices (one division per entry, not per lane
//                   and step).
//   k_kr_fold       when the tiles alone do not fill the chip the contraction axis (samples / tensor rows) is split: every split
//                   writes its own [split][rows][cols] partial, and the fold adds them in split order.  No floating-point
//                   atomics anywhere: two calls give the same bits.
// Row, column and contraction tails are zero-filled in LDS (exact: a zero term adds nothing), stores are guarded.
#include <algorithm>
#include <cstdint>

#include "hip_common.h"

namespace ccz {

namespace {

constexpr int KR_MAXV = 8;                           // views per call
constexpr int KR_NL = KR_MAXV - 1;                   // most views in a Khatri-Rao product
constexpr int64_t KR_MAXPROD = int64_t(1) << 24;     // most tensor entries
constexpr int KR_T = 64;                             // tile edge: tensor rows / samples / columns per workgroup
constexpr int KR_S = 32;                             // k_kr_moment: samples per staged chunk
constexpr int KR_KC = 32;                            // k_kr_apply: tensor rows per staged chunk
constexpr int KR_BW = 80;                            // LDS row stride of the B tile (80 % 32 == 16: the two rows of a half wave on disjoint banks)
constexpr int KR_MAXSPLIT = 64;                      // most splits of the contraction axis
constexpr size_t KR_LDS_MAX = size_t(48) << 10;

typedef double v4f64 __attribute__((ext_vector_type(4)));

// the views of one Khatri-Rao product, the last one's index fastest
struct KrSide {
  const double* p[KR_NL];
  int64_t ld[KR_NL];
  int d[KR_NL];
  int stride[KR_NL];     // prod of the later views' widths
  int nl;
  int rows;              // prod d
};

// ---- M = scale A' H_V --------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) k_kr_moment(KrSide A, const double* __restrict__ B, int64_t ldb, int C, int64_t n, int64_t sps,
                                                   int tc, int LW, double* __restrict__ dst, int64_t ldd, int64_t zstride, double scale) {
  extern __shared__ double kr_lds[];
  double* As = kr_lds;                    // KR_S x LW: the windows of the left views, side by side
  double* Bs = kr_lds + KR_S * LW;        // KR_S x KR_BW
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, li = lane & 15, lg = lane >> 4;
  const int r0 = int(blockIdx.x / tc) * KR_T, c0 = int(blockIdx.x % tc) * KR_T;
  const int rl = min(r0 + KR_T, A.rows) - 1;
  int off[KR_NL], q0[KR_NL], w[KR_NL];
  int o = 0;
#pragma unroll
  for (int i = 0; i < KR_NL; ++i) {
    off[i] = o; q0[i] = 0; w[i] = 0;
    if (i < A.nl) {
      q0[i] = r0 / A.stride[i];
      w[i] = min(rl / A.stride[i] - q0[i] + 1, A.d[i]);
      o += w[i];
    }
  }
  const int r = r0 + 16 * wave + li;
  const bool valid = r < A.rows;
  int idx[KR_NL];
#pragma unroll
  for (int i = 0; i < KR_NL; ++i) idx[i] = off[i] + ((valid && i < A.nl) ? (r / A.stride[i] - q0[i]) % A.d[i] : 0);
  const int nct = min(4, (C - c0 + 15) / 16);
  const int64_t sb = int64_t(blockIdx.z) * sps, se = min(n, sb + sps);
  const int sr = tid >> 5, sc = tid & 31;
  v4f64 acc[4];
#pragma unroll
  for (int ct = 0; ct < 4; ++ct) acc[ct] = v4f64{0.0, 0.0, 0.0, 0.0};
  for (int64_t s0 = sb; s0 < se; s0 += KR_S) {
    __syncthreads();
#pragma unroll
    for (int i = 0; i < KR_NL; ++i) {
      if (i >= A.nl) break;
      for (int t = sc; t < w[i]; t += 32) {
        const int g = (q0[i] + t) % A.d[i];
        for (int sl = sr; sl < KR_S; sl += 8) {
          const int64_t s = s0 + sl;
          As[sl * LW + off[i] + t] = s < se ? A.p[i][s * A.ld[i] + g] : 0.0;
        }
      }
    }
    for (int cc = sc; cc < KR_T; cc += 32) {
      const int col = c0 + cc;
      for (int sl = sr; sl < KR_S; sl += 8) {
        const int64_t s = s0 + sl;
        Bs[sl * KR_BW + cc] = (s < se && col < C) ? B[s * ldb + col] : 0.0;
      }
    }
    __syncthreads();
#pragma unroll 2
    for (int k4 = 0; k4 < KR_S; k4 += 4) {
      const double* ar = As + (k4 + lg) * LW;
      double av = ar[idx[0]];
#pragma unroll
      for (int i = 1; i < KR_NL; ++i)
        if (i < A.nl) av *= ar[idx[i]];
      av = valid ? av : 0.0;
      const double* br = Bs + (k4 + lg) * KR_BW + li;
#pragma unroll
      for (int ct = 0; ct < 4; ++ct)
        if (ct < nct) acc[ct] = __builtin_amdgcn_mfma_f64_16x16x4f64(av, br[16 * ct], acc[ct], 0, 0, 0);
    }
  }
  double* out = dst + int64_t(blockIdx.z) * zstride;
#pragma unroll
  for (int ct = 0; ct < 4; ++ct) {
    const int col = c0 + 16 * ct + li;
    if (ct >= nct || col >= C) continue;
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      const int row = r0 + 16 * wave + lg + 4 * g;
      if (row < A.rows) out[int64_t(row) * ldd + col] = scale * acc[ct][g];
    }
  }
}

// ---- T_(j): (outer, d_j, inner) -> (outer, inner, d_j) -------------------------------------------------------------------
__global__ void __launch_bounds__(256) k_kr_unfold(const double* __restrict__ T, int64_t total, int dj, int inner, double* __restrict__ Tp) {
  const int64_t e = int64_t(blockIdx.x) * 256 + threadIdx.x;
  if (e >= total) return;
  const int a = int(e % dj);
  const int64_t rp = e / dj, lo = rp % inner, hi = rp / inner;
  Tp[e] = T[(hi * dj + a) * inner + lo];
}

// ---- out = scale B_j T_(j) -------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) k_kr_apply(KrSide A, const double* __restrict__ T, int dj, int64_t n, int kps, int tc, int LW,
                                                  double* __restrict__ dst, int64_t ldd, int64_t zstride, double scale) {
  extern __shared__ double kr_lds[];
  double* As = kr_lds;                                   // KR_T samples x LW
  double* Ts = As + KR_T * LW;                           // KR_KC x KR_BW
  int* tix = reinterpret_cast<int*>(Ts + KR_KC * KR_BW); // KR_KC x 8: window index of tensor row kk in view i
  int* meta = tix + KR_KC * 8;                           // q0[8], w[8] of the chunk
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, li = lane & 15, lg = lane >> 4;
  const int64_t s0 = int64_t(blockIdx.x / tc) * KR_T;
  const int c0 = int(blockIdx.x % tc) * KR_T;
  const int kb = int(blockIdx.z) * kps, ke = min(A.rows, kb + kps);
  const int nct = min(4, (dj - c0 + 15) / 16);
  const int sr = tid >> 5, sc = tid & 31;
  v4f64 acc[4];
#pragma unroll
  for (int ct = 0; ct < 4; ++ct) acc[ct] = v4f64{0.0, 0.0, 0.0, 0.0};
  for (int k0 = kb; k0 < ke; k0 += KR_KC) {
    const int kl = min(k0 + KR_KC, ke) - 1;
    __syncthreads();
#pragma unroll
    for (int i = 0; i < KR_NL; ++i)
      if (tid == i) {
        int q = 0, ww = 0;
        if (i < A.nl) {
          q = k0 / A.stride[i];
          ww = min(kl / A.stride[i] - q + 1, A.d[i]);
        }
        meta[i] = q;
        meta[8 + i] = ww;
      }
    __syncthreads();
    int off[KR_NL], q0[KR_NL], w[KR_NL];
    int o = 0;
#pragma unroll
    for (int i = 0; i < KR_NL; ++i) {
      q0[i] = meta[i]; w[i] = meta[8 + i];
      off[i] = o; o += w[i];
    }
    {
      const int k = k0 + (tid >> 3), iv = tid & 7;
      int v = 0;
#pragma unroll
      for (int i = 0; i < KR_NL; ++i)
        if (i == iv && i < A.nl) v = off[i] + (k < ke ? (k / A.stride[i] - q0[i]) % A.d[i] : 0);
      tix[tid] = v;
    }
#pragma unroll
    for (int i = 0; i < KR_NL; ++i) {
      if (i >= A.nl) break;
      for (int t = sc; t < w[i]; t += 32) {
        const int g = (q0[i] + t) % A.d[i];
        for (int sl = sr; sl < KR_T; sl += 8) {
          const int64_t s = s0 + sl;
          As[sl * LW + off[i] + t] = s < n ? A.p[i][s * A.ld[i] + g] : 0.0;
        }
      }
    }
    for (int cc = sc; cc < KR_T; cc += 32) {
      const int col = c0 + cc;
      for (int kk = sr; kk < KR_KC; kk += 8) {
        const int k = k0 + kk;
        Ts[kk * KR_BW + cc] = (k < ke && col < dj) ? T[int64_t(k) * dj + col] : 0.0;
      }
    }
    __syncthreads();
    const double* ar = As + (16 * wave + li) * LW;
#pragma unroll 2
    for (int k4 = 0; k4 < KR_KC; k4 += 4) {
      const int kq = k4 + lg;
      const int* tr = tix + kq * 8;
      double av = ar[tr[0]];
#pragma unroll
      for (int i = 1; i < KR_NL; ++i)
        if (i < A.nl) av *= ar[tr[i]];
      av = k0 + kq < ke ? av : 0.0;
      const double* br = Ts + kq * KR_BW + li;
#pragma unroll
      for (int ct = 0; ct < 4; ++ct)
        if (ct < nct) acc[ct] = __builtin_amdgcn_mfma_f64_16x16x4f64(av, br[16 * ct], acc[ct], 0, 0, 0);
    }
  }
  double* out = dst + int64_t(blockIdx.z) * zstride;
#pragma unroll
  for (int ct = 0; ct < 4; ++ct) {
    const int col = c0 + 16 * ct + li;
    if (ct >= nct || col >= dj) continue;
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      const int64_t row = s0 + 16 * wave + lg + 4 * g;
      if (row < n) out[row * ldd + col] = scale * acc[ct][g];
    }
  }
}

// ---- out = scale (part[0] + part[1] + ..) in split order ------------------------------------------------------------------
__global__ void __launch_bounds__(256) k_kr_fold(const double* __restrict__ part, int split, int64_t rows, int cols, double scale,
                                                 double* __restrict__ out, int64_t ldo) {
  const int64_t e = int64_t(blockIdx.x) * 256 + threadIdx.x, total = rows * cols;
  if (e >= total) return;
  double s = 0.0;
  for (int z = 0; z < split; ++z) s += part[int64_t(z) * total + e];
  out[(e / cols) * ldo + e % cols] = scale * s;
}

// argument checks shared by the two entries; returns prod d_i
int64_t kr_check(const char* who, const ccz_view* H, int n_views, int64_t n) {
  if (n_views < 2 || n_views > KR_MAXV) fail(CCZ_EINVAL, "%s: n_views must be 2..%d, got %d", who, KR_MAXV, n_views);
  if (!H) fail(CCZ_EINVAL, "%s: null views", who);
  if (n < 1 || n > int64_t(1) << 40) fail(CCZ_EINVAL, "%s: bad row count %lld", who, (long long)n);
  int64_t prod = 1;
  for (int i = 0; i < n_views; ++i) {
    if (!H[i].data || H[i].cols < 1 || H[i].ld < H[i].cols) fail(CCZ_EINVAL, "%s: bad view %d", who, i);
    if (H[i].cols > KR_MAXPROD) fail(CCZ_EINVAL, "%s: the product of the views' widths exceeds 2^24", who);
    prod *= H[i].cols;
    if (prod > KR_MAXPROD) fail(CCZ_EINVAL, "%s: the product of the views' widths exceeds 2^24", who);
  }
  return prod;
}

// the Khatri-Rao side of all views but `skip`
KrSide kr_side(const ccz_view* H, int n_views, int skip) {
  KrSide A{};
  for (int i = 0; i < n_views; ++i) {
    if (i == skip) continue;
    A.p[A.nl] = static_cast<const double*>(H[i].data);
    A.ld[A.nl] = H[i].ld;
    A.d[A.nl] = int(H[i].cols);
    ++A.nl;
  }
  int s = 1;
  for (int i = A.nl - 1; i >= 0; --i) { A.stride[i] = s; s *= A.d[i]; }
  A.rows = s;
  for (int i = A.nl; i < KR_NL; ++i) { A.p[i] = nullptr; A.ld[i] = 0; A.d[i] = 1; A.stride[i] = 1; }
  return A;
}

// most window columns `span` consecutive tensor rows touch, over all views
int kr_window(const KrSide& A, int span) {
  int lw = 0;
  for (int i = 0; i < A.nl; ++i) lw += std::min(A.d[i], (span - 1) / A.stride[i] + 2);
  return lw;
}

// splits of a contraction axis of `chunks` chunks so that tiles x splits fills the chip
int kr_split(ccz_ctx* c, int64_t tiles, int64_t chunks) {
  const int64_t want = 2 * int64_t(impl(c)->props.multiProcessorCount);
  if (tiles >= want) return 1;
  return int(std::max<int64_t>(1, std::min<int64_t>({(want + tiles - 1) / tiles, chunks, KR_MAXSPLIT})));
}

void kr_fold(ccz_ctx* c, const double* part, int split, int64_t rows, int cols, double scale, double* out, int64_t ldo) {
  const int64_t total = rows * cols;
  hipLaunchKernelGGL(k_kr_fold, dim3(unsigned((total + 255) / 256)), dim3(256), 0, stream(c), part, split, rows, cols, scale, out, ldo);
  CCZ_LAUNCH_CHECK();
}

}  // namespace

void kr_moment_impl(ccz_ctx* c, const ccz_view* H, int n_views, int64_t n, double scale, double* M) {
  const int64_t prod = kr_check("kr_moment", H, n_views, n);
  if (!M) fail(CCZ_EINVAL, "kr_moment: null output");
  const KrSide A = kr_side(H, n_views, n_views - 1);
  const int C = int(H[n_views - 1].cols);
  const int64_t R = prod / C;
  int lw = kr_window(A, KR_T);
  lw += (16 - lw % 32 + 32) % 32;                       // == 16 mod 32
  const size_t lds = size_t(KR_S) * (lw + KR_BW) * sizeof(double);
  if (lds > KR_LDS_MAX) fail(CCZ_EUNSUP, "kr_moment: window of %d columns does not fit", lw);
  const int tc = (C + KR_T - 1) / KR_T;
  const int64_t tiles = ((R + KR_T - 1) / KR_T) * tc;
  const int64_t chunks = (n + KR_S - 1) / KR_S;
  int split = kr_split(c, tiles, chunks);
  const int64_t sps = (chunks + split - 1) / split * KR_S;
  split = int((n + sps - 1) / sps);
  const double* B = static_cast<const double*>(H[n_views - 1].data);
  const int64_t ldb = H[n_views - 1].ld;
  if (split == 1) {
    hipLaunchKernelGGL(k_kr_moment, dim3(unsigned(tiles), 1, 1), dim3(256), lds, stream(c), A, B, ldb, C, n, sps, tc, lw, M, int64_t(C), int64_t(0), scale);
    CCZ_LAUNCH_CHECK();
    return;
  }
  DBuf part(c, int64_t(split) * prod);
  hipLaunchKernelGGL(k_kr_moment, dim3(unsigned(tiles), 1, unsigned(split)), dim3(256), lds, stream(c), A, B, ldb, C, n, sps, tc, lw, part.get(), int64_t(C), prod, 1.0);
  CCZ_LAUNCH_CHECK();
  kr_fold(c, part, split, R, C, scale, M, C);
}

void kr_apply_impl(ccz_ctx* c, const ccz_view* H, int n_views, int64_t n, const double* T, int mode, double scale, double* out,
                   int64_t ldo) {
  const int64_t prod = kr_check("kr_apply", H, n_views, n);
  if (mode < 0 || mode >= n_views) fail(CCZ_EINVAL, "kr_apply: mode must be 0..%d, got %d", n_views - 1, mode);
  const int dj = int(H[mode].cols);
  if (!T || !out || ldo < dj) fail(CCZ_EINVAL, "kr_apply: bad argument");
  const KrSide A = kr_side(H, n_views, mode);
  int lw = kr_window(A, KR_KC);
  lw |= 1;                                              // odd: the 16 samples of a half wave read one column on 16 banks
  const size_t lds = (size_t(KR_T) * lw + size_t(KR_KC) * KR_BW) * sizeof(double) + (KR_KC * 8 + 16) * sizeof(int);
  if (lds > KR_LDS_MAX) fail(CCZ_EUNSUP, "kr_apply: window of %d columns does not fit", lw);
  DBuf tp;
  const double* Tj = T;
  if (mode != n_views - 1) {
    int64_t inner = 1;
    for (int i = mode + 1; i < n_views; ++i) inner *= H[i].cols;
    tp = DBuf(c, prod);
    hipLaunchKernelGGL(k_kr_unfold, dim3(unsigned((prod + 255) / 256)), dim3(256), 0, stream(c), T, prod, dj, int(inner), tp.get());
    CCZ_LAUNCH_CHECK();
    Tj = tp.get();
  }
  const int tc = (dj + KR_T - 1) / KR_T;
  const int64_t tiles = ((n + KR_T - 1) / KR_T) * tc;
  if (tiles > int64_t(0x7fffffff)) fail(CCZ_EINVAL, "kr_apply: too many rows");
  const int64_t chunks = (int64_t(A.rows) + KR_KC - 1) / KR_KC;
  int split = kr_split(c, tiles, chunks);
  const int kps = int((chunks + split - 1) / split * KR_KC);
  split = (A.rows + kps - 1) / kps;
  if (split == 1) {
    hipLaunchKernelGGL(k_kr_apply, dim3(unsigned(tiles), 1, 1), dim3(256), lds, stream(c), A, Tj, dj, n, kps, tc, lw, out, ldo, int64_t(0), scale);
    CCZ_LAUNCH_CHECK();
    return;
  }
  DBuf part(c, int64_t(split) * n * dj);
  hipLaunchKernelGGL(k_kr_apply, dim3(unsigned(tiles), 1, unsigned(split)), dim3(256), lds, stream(c), A, Tj, dj, n, kps, tc, lw, part.get(), int64_t(dj), n * dj, 1.0);
  CCZ_LAUNCH_CHECK();
  kr_fold(c, part, split, n, dj, scale, out, ldo);
}

}  // namespace ccz
