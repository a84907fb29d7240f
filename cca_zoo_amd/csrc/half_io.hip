// The 2-byte formats of the deep objectives (CCZ_BF16 / CCZ_F16) as an input / output FORMAT in front of the float32 routes.
//
// K1's split route reads half rows itself (gram_split.hip: k_split_bf16x2<T>).  Every other route is served here, by a row-chunk
// adapter: rows [r0, r0 + rows) of the half views are widened exactly into float32 scratch from the handle's pool (k_widen_half),
// the UNCHANGED float32 implementation runs on that scratch, and where it writes n x d rows (gradients, projections) they are
// rounded once, to nearest even, into the caller's half rows (k_narrow_half).  Chunks are sized so the scratch stays within
// CCZ_HALF_SCRATCH_MB; a batch that fits is one chunk -- a DCCA batch costs one small launch each way.
//
//   moments     add over chunks through the `accumulate` flag of the float32 call, each chunk with its own pilot (as streamed
//               host views do)
//   gradients,  rows are independent given Gamma, the mean and the state; the float32 backward wants at least 2 rows, so a
//   projections 1-row tail is folded into its neighbour
//
// Both kernels are HBM-bound streams: a lane handles 16 bytes of half elements (8 of them: 16 bytes in and 32 out, or the
// reverse); the last partial group of a row and rows that do not start on 16 bytes go element by element.
#include <algorithm>

#include "hip_common.h"
#include "half_cvt.h"

namespace ccz {

namespace {

constexpr int HIO_V = 8;                 // views per launch

typedef unsigned int hio_v4u32 __attribute__((ext_vector_type(4)));
typedef float hio_v4f32 __attribute__((ext_vector_type(4)));

struct HalfIoArgs {
  const void* src[HIO_V];
  void* dst[HIO_V];
  int64_t cols[HIO_V], lds[HIO_V], ldd[HIO_V];
  int vec[HIO_V];                        // bit 0: the half rows take 16-byte accesses, bit 1: the float32 rows do
};

// float32 dst rows <- half src rows, exactly.  grid = (blocks over rows x groups of 8 columns, views)
template <typename T>
__global__ __launch_bounds__(256) void k_widen_half(HalfIoArgs a, int64_t rows) {
  const int v = blockIdx.y;
  const T* __restrict__ S = static_cast<const T*>(a.src[v]);
  float* __restrict__ D = static_cast<float*>(a.dst[v]);
  const int64_t cols = a.cols[v], lds = a.lds[v], ldd = a.ldd[v], groups = (cols + 7) / 8, total = rows * groups;
  const bool vs = a.vec[v] & 1, vd = a.vec[v] & 2;
  for (int64_t e = int64_t(blockIdx.x) * 256 + threadIdx.x; e < total; e += int64_t(gridDim.x) * 256) {
    const int64_t row = e / groups, c = (e - row * groups) * 8;
    const T* s = S + row * lds + c;
    float* d = D + row * ldd + c;
    if (c + 8 <= cols) {
      float x[8];
      if (vs) {
        const hio_v4u32 w = __builtin_nontemporal_load(reinterpret_cast<const hio_v4u32*>(s));          // read once
#pragma unroll
        for (int k = 0; k < 8; ++k) x[k] = widen(T{uint16_t(w[k >> 1] >> (16 * (k & 1)))});
      } else {
#pragma unroll
        for (int k = 0; k < 8; ++k) x[k] = widen(s[k]);
      }
      if (vd) {
        *reinterpret_cast<hio_v4f32*>(d) = hio_v4f32{x[0], x[1], x[2], x[3]};
        *reinterpret_cast<hio_v4f32*>(d + 4) = hio_v4f32{x[4], x[5], x[6], x[7]};
      } else {
#pragma unroll
        for (int k = 0; k < 8; ++k) d[k] = x[k];
      }
    } else {
      for (int k = 0; c + k < cols; ++k) d[k] = widen(s[k]);
    }
  }
}

// half dst rows <- float32 src rows, rounded to nearest even.  Same grid.
template <typename T>
__global__ __launch_bounds__(256) void k_narrow_half(HalfIoArgs a, int64_t rows) {
  const int v = blockIdx.y;
  const float* __restrict__ S = static_cast<const float*>(a.src[v]);
  T* __restrict__ D = static_cast<T*>(a.dst[v]);
  const int64_t cols = a.cols[v], lds = a.lds[v], ldd = a.ldd[v], groups = (cols + 7) / 8, total = rows * groups;
  const bool vd = a.vec[v] & 1, vs = a.vec[v] & 2;
  for (int64_t e = int64_t(blockIdx.x) * 256 + threadIdx.x; e < total; e += int64_t(gridDim.x) * 256) {
    const int64_t row = e / groups, c = (e - row * groups) * 8;
    const float* s = S + row * lds + c;
    T* d = D + row * ldd + c;
    if (c + 8 <= cols) {
      float x[8];
      if (vs) {
        const hio_v4f32 lo = *reinterpret_cast<const hio_v4f32*>(s), hi = *reinterpret_cast<const hio_v4f32*>(s + 4);
#pragma unroll
        for (int k = 0; k < 4; ++k) { x[k] = lo[k]; x[4 + k] = hi[k]; }
      } else {
#pragma unroll
        for (int k = 0; k < 8; ++k) x[k] = s[k];
      }
      if (vd) {
        hio_v4u32 w;
#pragma unroll
        for (int k = 0; k < 4; ++k) w[k] = unsigned(narrow<T>(x[2 * k]).bits) | (unsigned(narrow<T>(x[2 * k + 1]).bits) << 16);
        *reinterpret_cast<hio_v4u32*>(d) = w;
      } else {
#pragma unroll
        for (int k = 0; k < 8; ++k) d[k] = narrow<T>(x[k]);
      }
    } else {
      for (int k = 0; c + k < cols; ++k) d[k] = narrow<T>(s[k]);
    }
  }
}

bool on16(const void* p, int64_t ld, int64_t elems_per_16) { return reinterpret_cast<uintptr_t>(p) % 16 == 0 && ld % elems_per_16 == 0; }

// one launch per HIO_V views; widen: half -> float32, else the reverse
void launch_io(ccz_ctx* c, int dtype, bool widen_dir, const HalfIoArgs& a, int m, int64_t rows) {
  int64_t most = 0;
  for (int v = 0; v < m; ++v) most = std::max(most, rows * ((a.cols[v] + 7) / 8));
  const unsigned blocks = unsigned(std::min<int64_t>(2048, std::max<int64_t>(1, (most + 255) / 256)));
  const dim3 grid(blocks, unsigned(m));
  if (widen_dir) {
    if (dtype == CCZ_BF16) hipLaunchKernelGGL(k_widen_half<bf16_t>, grid, dim3(256), 0, stream(c), a, rows);
    else hipLaunchKernelGGL(k_widen_half<f16_t>, grid, dim3(256), 0, stream(c), a, rows);
  } else {
    if (dtype == CCZ_BF16) hipLaunchKernelGGL(k_narrow_half<bf16_t>, grid, dim3(256), 0, stream(c), a, rows);
    else hipLaunchKernelGGL(k_narrow_half<f16_t>, grid, dim3(256), 0, stream(c), a, rows);
  }
  CCZ_LAUNCH_CHECK();
}

int64_t round4(int64_t x) { return (x + 3) / 4 * 4; }

}  // namespace

int64_t half_row_bytes(const int64_t* cols, int m) {
  int64_t b = 0;
  for (int v = 0; v < m; ++v) b += round4(cols[v]) * 4;
  return b;
}

int64_t half_chunk_rows(int64_t row_bytes, int64_t n) {
  const double budget = std::max(4096.0, env::live(env::HALF_SCRATCH_MB) * 1048576.0);
  const double fit = budget / double(std::max<int64_t>(1, row_bytes));
  if (fit >= double(n)) return n;
  return std::max<int64_t>(2, int64_t(fit));
}

int64_t half_next_chunk(int64_t r0, int64_t chunk, int64_t n) {
  const int64_t rows = std::min(chunk, n - r0);
  return n - r0 - rows == 1 ? rows + 1 : rows;
}

void half_stage(ccz_ctx* c, const int64_t* cols, int m, int64_t rows, HalfStage* st) {
  if (m < 1 || m > HALF_MAXV) fail(CCZ_EUNSUP, "half views: 1 .. %d views are supported, got %d", HALF_MAXV, m);
  int64_t per_row = 0;
  for (int v = 0; v < m; ++v) per_row += round4(cols[v]);
  st->buf = PoolBuf<float>(c, per_row * rows);
  st->m = m;
  st->rows = rows;
  int64_t off = 0;
  for (int v = 0; v < m; ++v) {
    st->fv[v] = ccz_view{st->buf.get() + off, cols[v], round4(cols[v])};     // (every view starts on 16 bytes: the offsets are multiples of 4 floats)
    off += round4(cols[v]) * rows;
  }
}

void half_widen(ccz_ctx* c, int dtype, const ccz_view* views, int m, int64_t r0, int64_t rows, const HalfStage& st) {
  if (!is_half_dtype(dtype) || m != st.m || rows > st.rows) fail(CCZ_EINVAL, "half views: bad staging call");
  if (rows < 1) return;
  for (int v0 = 0; v0 < m; v0 += HIO_V) {
    HalfIoArgs a{};
    const int k = std::min(HIO_V, m - v0);
    for (int v = 0; v < k; ++v) {
      const ccz_view& hv = views[v0 + v];
      a.src[v] = static_cast<const char*>(hv.data) + r0 * hv.ld * 2;
      a.dst[v] = const_cast<void*>(st.fv[v0 + v].data);
      a.cols[v] = hv.cols; a.lds[v] = hv.ld; a.ldd[v] = st.fv[v0 + v].ld;
      a.vec[v] = (on16(a.src[v], hv.ld, 8) ? 1 : 0) | (on16(a.dst[v], a.ldd[v], 4) ? 2 : 0);
    }
    launch_io(c, dtype, true, a, k, rows);
  }
}

// rows [0, rows) of the staged float32 views -> rows [r0, r0 + rows) of dst[v] (leading dimension ldd[v]; null: that view is skipped)
void half_narrow(ccz_ctx* c, int dtype, const HalfStage& st, int64_t rows, void* const* dst, const int64_t* ldd, int64_t r0) {
  if (!is_half_dtype(dtype) || rows > st.rows) fail(CCZ_EINVAL, "half views: bad staging call");
  if (rows < 1) return;
  HalfIoArgs a{};
  int k = 0;
  for (int v = 0; v <= st.m; ++v) {
    if (v < st.m && dst[v]) {
      a.src[k] = st.fv[v].data;
      a.dst[k] = static_cast<char*>(dst[v]) + r0 * ldd[v] * 2;
      a.cols[k] = st.fv[v].cols; a.lds[k] = st.fv[v].ld; a.ldd[k] = ldd[v];
      a.vec[k] = (on16(a.dst[k], ldd[v], 8) ? 1 : 0) | (on16(a.src[k], a.lds[k], 4) ? 2 : 0);
      ++k;
    }
    if (k == HIO_V || (v == st.m && k > 0)) {
      launch_io(c, dtype, false, a, k, rows);
      k = 0;
    }
  }
}

void half_moments(ccz_ctx* c, int dtype, const ccz_view* views, int n_views, int64_t n, double* moments, int pilot_mode, bool time_it) {
  if (n_views > HALF_MAXV) fail(CCZ_EUNSUP, "moments: at most %d half views on the fp32 route, got %d", HALF_MAXV, n_views);
  int64_t cols[HALF_MAXV];
  for (int v = 0; v < n_views; ++v) cols[v] = views[v].cols;
  const int64_t chunk = half_chunk_rows(half_row_bytes(cols, n_views), n);
  HalfStage st;
  half_stage(c, cols, n_views, chunk < n ? chunk + 1 : n, &st);
  double gram_ms = 0.0, colsum_ms = 0.0;
  for (int64_t r0 = 0; r0 < n;) {
    const int64_t rows = half_next_chunk(r0, chunk, n);
    half_widen(c, dtype, views, n_views, r0, rows, st);
    moments_impl(c, CCZ_F32, st.fv, n_views, rows, true, moments, true, pilot_mode, time_it);
    gram_ms += c->last_gram_ms;
    colsum_ms += c->last_colsum_ms;
    r0 += rows;
  }
  c->last_gram_ms = gram_ms;
  c->last_colsum_ms = colsum_ms;
}

}  // namespace ccz
