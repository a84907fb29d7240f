// HIP (gfx950 / CDNA4) implementation of the device-op interface in ops.h: elementwise / layout kernels and
// the small reductions (transpose ... gather_rows), float64, row-major.
#include <algorithm>
#include <vector>

#include "hip_common.h"
#include "reduce.h"
#include "rng_hash.h"

namespace ccz {

// ===========================================================================
// elementwise / layout kernels
// ===========================================================================
__global__ void k_transpose(int64_t rows, int64_t cols, const double* __restrict__ in, int64_t ldi,
                            double* __restrict__ out, int64_t ldo) {
  __shared__ double t[32][33];
  const int64_t r0 = int64_t(blockIdx.y) * 32, c0 = int64_t(blockIdx.x) * 32;
  for (int i = threadIdx.y; i < 32; i += 8) {
    const int64_t r = r0 + i, cc = c0 + threadIdx.x;
    if (r < rows && cc < cols) t[i][threadIdx.x] = in[r * ldi + cc];
  }
  __syncthreads();
  for (int i = threadIdx.y; i < 32; i += 8) {
    const int64_t orow = c0 + i, ocol = r0 + threadIdx.x;   // out is cols x rows
    if (orow < cols && ocol < rows) out[orow * ldo + ocol] = t[threadIdx.x][i];
  }
}

void transpose(ccz_ctx* c, int64_t rows, int64_t cols, const double* in, int64_t ldi, double* out, int64_t ldo) {
  if (rows <= 0 || cols <= 0) return;
  const int64_t by = (rows + 31) / 32;
  for (int64_t y0 = 0; y0 < by; y0 += 65535) {   // grid.y limit
    const int64_t ny = std::min<int64_t>(65535, by - y0);
    dim3 grid((unsigned)((cols + 31) / 32), (unsigned)ny);
    hipLaunchKernelGGL(k_transpose, grid, dim3(32, 8), 0, stream(c), rows - y0 * 32, cols, in + y0 * 32 * ldi, ldi,
                       out + y0 * 32, ldo);
  }
  CCZ_LAUNCH_CHECK();
}

#define CCZ_GRID2D(rows, cols) \
  dim3 grid((unsigned)std::min<int64_t>(((rows) * (cols) + 255) / 256, 1 << 20)); \
  const int64_t total = (rows) * (cols)

__global__ void k_copy2d(int64_t total, int64_t cols, const double* __restrict__ in, int64_t ldi,
                         double* __restrict__ out, int64_t ldo) {
  for (int64_t i = int64_t(blockIdx.x) * blockDim.x + threadIdx.x; i < total; i += int64_t(gridDim.x) * blockDim.x) {
    const int64_t r = i / cols, cc = i - r * cols;
    out[r * ldo + cc] = in[r * ldi + cc];
  }
}
void copy2d(ccz_ctx* c, int64_t rows, int64_t cols, const double* in, int64_t ldi, double* out, int64_t ldo) {
  if (rows <= 0 || cols <= 0 || (in == out && ldi == ldo)) return;
  if (in == out) fail(CCZ_EINVAL, "copy2d: in-place with different strides");
  CCZ_GRID2D(rows, cols);
  hipLaunchKernelGGL(k_copy2d, grid, dim3(256), 0, stream(c), total, cols, in, ldi, out, ldo);
  CCZ_LAUNCH_CHECK();
}

__global__ void k_axpby2d(int64_t total, int64_t cols, double alpha, double* __restrict__ A, int64_t lda, double beta,
                          const double* __restrict__ B, int64_t ldb) {
  for (int64_t i = int64_t(blockIdx.x) * blockDim.x + threadIdx.x; i < total; i += int64_t(gridDim.x) * blockDim.x) {
    const int64_t r = i / cols, cc = i - r * cols;
    double v = alpha * A[r * lda + cc];
    if (B) v += beta * B[r * ldb + cc];
    A[r * lda + cc] = v;
  }
}
void axpby2d(ccz_ctx* c, int64_t rows, int64_t cols, double alpha, double* A, int64_t lda, double beta, const double* B,
             int64_t ldb) {
  if (rows <= 0 || cols <= 0) return;
  if (beta == 0.0) B = nullptr;
  CCZ_GRID2D(rows, cols);
  hipLaunchKernelGGL(k_axpby2d, grid, dim3(256), 0, stream(c), total, cols, alpha, A, lda, beta, B, ldb);
  CCZ_LAUNCH_CHECK();
}

__global__ void k_fill2d(int64_t total, int64_t cols, double* __restrict__ A, int64_t lda, double v) {
  for (int64_t i = int64_t(blockIdx.x) * blockDim.x + threadIdx.x; i < total; i += int64_t(gridDim.x) * blockDim.x) {
    const int64_t r = i / cols, cc = i - r * cols;
    A[r * lda + cc] = v;
  }
}
void fill2d(ccz_ctx* c, int64_t rows, int64_t cols, double* A, int64_t lda, double v) {
  if (rows <= 0 || cols <= 0) return;
  CCZ_GRID2D(rows, cols);
  hipLaunchKernelGGL(k_fill2d, grid, dim3(256), 0, stream(c), total, cols, A, lda, v);
  CCZ_LAUNCH_CHECK();
}

__global__ void k_add_diag(int64_t d, double* __restrict__ A, int64_t lda, double v) {
  const int64_t i = int64_t(blockIdx.x) * blockDim.x + threadIdx.x;
  if (i < d) A[i * lda + i] += v;
}
void add_diag(ccz_ctx* c, int64_t d, double* A, int64_t lda, double v) {
  if (d <= 0) return;
  hipLaunchKernelGGL(k_add_diag, dim3((unsigned)((d + 255) / 256)), dim3(256), 0, stream(c), d, A, lda, v);
  CCZ_LAUNCH_CHECK();
}

__global__ void k_scale_cols(int64_t total, int64_t cols, double* __restrict__ A, int64_t lda,
                             const double* __restrict__ v, int mode) {
  for (int64_t i = int64_t(blockIdx.x) * blockDim.x + threadIdx.x; i < total; i += int64_t(gridDim.x) * blockDim.x) {
    const int64_t r = i / cols, cc = i - r * cols;
    const double f = mode == 0 ? v[cc] : (mode == 1 ? 1.0 / v[cc] : 1.0 / sqrt(v[cc]));
    A[r * lda + cc] *= f;
  }
}
void scale_cols(ccz_ctx* c, int64_t rows, int64_t cols, double* A, int64_t lda, const double* v, int mode) {
  if (rows <= 0 || cols <= 0) return;
  CCZ_GRID2D(rows, cols);
  hipLaunchKernelGGL(k_scale_cols, grid, dim3(256), 0, stream(c), total, cols, A, lda, v, mode);
  CCZ_LAUNCH_CHECK();
}

// lower tile (bi > bj) <- transpose of upper tile (bj, bi) through LDS; diagonal tiles in place
__global__ void k_mirror_upper(int64_t d, double* __restrict__ A, int64_t lda) {
  __shared__ double t[32][33];
  const int64_t bi = blockIdx.y, bj = blockIdx.x;
  if (bi < bj) return;
  const int64_t r0 = bj * 32, c0 = bi * 32;   // source tile: rows of block bj, cols of block bi (upper)
  for (int i = threadIdx.y; i < 32; i += 8) {
    const int64_t r = r0 + i, cc = c0 + threadIdx.x;
    if (r < d && cc < d) t[i][threadIdx.x] = A[r * lda + cc];
  }
  __syncthreads();
  for (int i = threadIdx.y; i < 32; i += 8) {
    const int64_t r = c0 + i, cc = r0 + threadIdx.x;   // destination (lower): A[r][cc] = A[cc][r]
    if (r < d && cc < d && r > cc) A[r * lda + cc] = t[threadIdx.x][i];
  }
}
void mirror_upper(ccz_ctx* c, int64_t d, double* A, int64_t lda) {
  if (d <= 0) return;
  const unsigned nb = (unsigned)((d + 31) / 32);
  hipLaunchKernelGGL(k_mirror_upper, dim3(nb, nb), dim3(32, 8), 0, stream(c), d, A, lda);
  CCZ_LAUNCH_CHECK();
}

template <bool PACK>
__global__ void k_pack_upper(int64_t d, double* __restrict__ A, int64_t lda, double* __restrict__ packed) {
  const int64_t i = blockIdx.y;
  const int64_t j = i + int64_t(blockIdx.x) * blockDim.x + threadIdx.x;
  if (j >= d) return;
  const int64_t off = i * d - (i * (i - 1)) / 2 + (j - i);
  if (PACK) packed[off] = A[i * lda + j]; else A[i * lda + j] = packed[off];
}
void pack_upper(ccz_ctx* c, int64_t d, const double* A, int64_t lda, double* packed) {
  if (d <= 0) return;
  if (d > 65535) fail(CCZ_EUNSUP, "pack_upper: d too large");
  hipLaunchKernelGGL(k_pack_upper<true>, dim3((unsigned)((d + 255) / 256), (unsigned)d), dim3(256), 0, stream(c), d,
                     const_cast<double*>(A), lda, packed);
  CCZ_LAUNCH_CHECK();
}
void unpack_upper(ccz_ctx* c, int64_t d, const double* packed, double* A, int64_t lda) {
  if (d <= 0) return;
  if (d > 65535) fail(CCZ_EUNSUP, "unpack_upper: d too large");
  hipLaunchKernelGGL(k_pack_upper<false>, dim3((unsigned)((d + 255) / 256), (unsigned)d), dim3(256), 0, stream(c), d, A,
                     lda, const_cast<double*>(packed));
  CCZ_LAUNCH_CHECK();
}

__global__ void k_cov_block(int64_t total, int64_t cols, const double* __restrict__ G, int64_t D,
                            const double* __restrict__ s, double inv_n, int centre, double alpha, int64_t r0,
                            int64_t c0, double* __restrict__ out, int64_t ldo) {
  for (int64_t i = int64_t(blockIdx.x) * blockDim.x + threadIdx.x; i < total; i += int64_t(gridDim.x) * blockDim.x) {
    const int64_t r = i / cols, cc = i - r * cols;
    // K1 fills upper-triangular tiles only: read every element from the upper triangle
    const int64_t gr = r0 + r, gc = c0 + cc;
    double v = gr <= gc ? G[gr * D + gc] : G[gc * D + gr];
    if (centre) v -= s[gr] * s[gc] * inv_n;
    out[r * ldo + cc] = alpha * v;
  }
}
void cov_block(ccz_ctx* c, const double* G, int64_t D, const double* s, int64_t n, bool centre, double alpha,
               int64_t r0, int64_t rows, int64_t c0, int64_t cols, double* out, int64_t ldo) {
  if (rows <= 0 || cols <= 0) return;
  CCZ_GRID2D(rows, cols);
  hipLaunchKernelGGL(k_cov_block, grid, dim3(256), 0, stream(c), total, cols, G, D, s, 1.0 / double(n), centre ? 1 : 0,
                     alpha, r0, c0, out, ldo);
  CCZ_LAUNCH_CHECK();
}

__global__ void k_randn(int64_t total, int64_t cols, double* __restrict__ A, int64_t lda, uint64_t seed) {
  for (int64_t i = int64_t(blockIdx.x) * blockDim.x + threadIdx.x; i < total; i += int64_t(gridDim.x) * blockDim.x) {
    const int64_t r = i / cols, cc = i - r * cols;
    A[r * lda + cc] = hash_normal(seed, uint64_t(i));
  }
}
void randn_fill(ccz_ctx* c, int64_t rows, int64_t cols, double* A, int64_t lda, uint64_t seed) {
  if (rows <= 0 || cols <= 0) return;
  CCZ_GRID2D(rows, cols);
  hipLaunchKernelGGL(k_randn, grid, dim3(256), 0, stream(c), total, cols, A, lda, seed);
  CCZ_LAUNCH_CHECK();
}

// ===========================================================================
// reductions
// ===========================================================================
__global__ void k_col_sqnorms(int64_t rows, int64_t cols, const double* __restrict__ A, int64_t lda,
                              double* __restrict__ out, int64_t rows_per_block) {
  const int64_t r0 = int64_t(blockIdx.x) * rows_per_block;
  const int64_t r1 = min(rows, r0 + rows_per_block);
  for (int64_t j = threadIdx.x; j < cols; j += blockDim.x) {
    double acc = 0.0;
    for (int64_t r = r0; r < r1; ++r) { const double v = A[r * lda + j]; acc += v * v; }
    unsafeAtomicAdd(&out[j], acc);
  }
}
void col_sqnorms(ccz_ctx* c, int64_t rows, int64_t cols, const double* A, int64_t lda, double* out) {
  if (cols <= 0) return;
  zero(c, out, size_t(cols) * 8);
  if (rows <= 0) return;
  const int64_t rpb = 64;
  hipLaunchKernelGGL(k_col_sqnorms, dim3((unsigned)((rows + rpb - 1) / rpb)), dim3(256), 0, stream(c), rows, cols, A,
                     lda, out, rpb);
  CCZ_LAUNCH_CHECK();
}

__global__ void k_row_abs_sums(int64_t cols, const double* __restrict__ A, int64_t lda, double* __restrict__ out) {
  __shared__ double red[8];
  const double* a = A + int64_t(blockIdx.x) * lda;
  double acc = 0.0;
  for (int64_t j = threadIdx.x; j < cols; j += blockDim.x) acc += fabs(a[j]);
  acc = block_sum_dyn(acc, red);
  if (threadIdx.x == 0) out[blockIdx.x] = acc;
}
double norm_inf(ccz_ctx* c, int64_t rows, int64_t cols, const double* A, int64_t lda) {
  if (rows <= 0 || cols <= 0) return 0.0;
  DBuf tmp(c, rows);
  hipLaunchKernelGGL(k_row_abs_sums, dim3((unsigned)rows), dim3(256), 0, stream(c), cols, A, lda, tmp.get());
  CCZ_LAUNCH_CHECK();
  std::vector<double> h(rows);
  d2h(c, h.data(), tmp, size_t(rows) * 8);
  double best = 0.0;
  for (double v : h)
    if (!(v <= best)) best = v;  // NaN propagates
  return best;
}

__global__ void k_row_dots(int64_t cols, const double* __restrict__ A, int64_t lda, const double* __restrict__ B,
                           int64_t ldb, double* __restrict__ out) {
  __shared__ double red[8];
  const double* a = A + int64_t(blockIdx.x) * lda;
  const double* b = B + int64_t(blockIdx.x) * ldb;
  double acc = 0.0;
  for (int64_t j = threadIdx.x; j < cols; j += blockDim.x) acc += a[j] * b[j];
  acc = block_sum_dyn(acc, red);
  if (threadIdx.x == 0) out[blockIdx.x] = acc;
}
void row_dots(ccz_ctx* c, int64_t rows, int64_t cols, const double* A, int64_t lda, const double* B, int64_t ldb,
              double* out) {
  if (rows <= 0) return;
  hipLaunchKernelGGL(k_row_dots, dim3((unsigned)rows), dim3(256), 0, stream(c), cols, A, lda, B, ldb, out);
  CCZ_LAUNCH_CHECK();
}

__global__ void k_gather_rows(int64_t total, int64_t cols, const double* __restrict__ in, int64_t ldi,
                              const int64_t* __restrict__ perm, const double* __restrict__ scale,
                              double* __restrict__ out, int64_t ldo) {
  for (int64_t i = int64_t(blockIdx.x) * blockDim.x + threadIdx.x; i < total; i += int64_t(gridDim.x) * blockDim.x) {
    const int64_t r = i / cols, cc = i - r * cols;
    out[r * ldo + cc] = in[perm[r] * ldi + cc] * (scale ? scale[r] : 1.0);
  }
}
void gather_rows(ccz_ctx* c, int64_t rows, int64_t cols, const double* in, int64_t ldi, const int64_t* perm_host,
                 const double* scale_host, double* out, int64_t ldo) {
  if (rows <= 0 || cols <= 0) return;
  DBuf pd(c, rows), sd(c, scale_host ? rows : 0);
  h2d(c, pd.get(), perm_host, size_t(rows) * 8);
  if (scale_host) h2d(c, sd.get(), scale_host, size_t(rows) * 8);
  CCZ_GRID2D(rows, cols);
  hipLaunchKernelGGL(k_gather_rows, grid, dim3(256), 0, stream(c), total, cols, in, ldi,
                     reinterpret_cast<const int64_t*>(pd.get()), scale_host ? sd.get() : nullptr, out, ldo);
  CCZ_LAUNCH_CHECK();
}

}  // namespace ccz
