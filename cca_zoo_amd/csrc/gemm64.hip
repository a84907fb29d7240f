// HIP (gfx950 / CDNA4) implementation of the device-op interface in ops.h: gemm, gemm_ex, gemm_mixed.
//
// Float64 dense linear algebra on d x d (d <= ~16k) blocks that lives AFTER the Gram reduction: it is latency /
// launch bound, not on the MFMA or HBM roofline (DESIGN.md "solver stage").  The GEMM uses the fp64 matrix pipe
// (v_mfma_f64_16x16x4_f64); products that gemm64_big.hip, gemm64_skinny.hip or gemm_big.hip take go there.
#include <algorithm>

#include "hip_common.h"

namespace ccz {

// ===========================================================================
// GEMM on the matrix pipe: 64x64 block tile, 4 waves (2x2), each wave 2x2 MFMA 16x16x4
// ===========================================================================
typedef double v4f64 __attribute__((ext_vector_type(4)));
typedef float v4f32 __attribute__((ext_vector_type(4)));

template <typename T> struct Mfma16;
template <> struct Mfma16<double> {
  typedef v4f64 acc_t;
  static __device__ __forceinline__ acc_t run(double a, double b, acc_t c) {
    return __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, c, 0, 0, 0);
  }
  // C/D layout of v_mfma_f64_16x16x4_f64: col = lane & 15, row = (lane >> 4) + 4 * reg
  static __device__ __forceinline__ int row(int lane, int reg) { return (lane >> 4) + 4 * reg; }
};
template <> struct Mfma16<float> {
  typedef v4f32 acc_t;
  static __device__ __forceinline__ acc_t run(float a, float b, acc_t c) {
    return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0);
  }
  // C/D layout of v_mfma_f32_16x16x4_f32: col = lane & 15, row = 4 * (lane >> 4) + reg
  static __device__ __forceinline__ int row(int lane, int reg) { return 4 * (lane >> 4) + reg; }
};

constexpr int GB = 64;   // block tile edge
constexpr int GK = 16;   // k-step
constexpr int GP = 4;    // LDS row padding (elements)

// C = alpha * (op(A) op(B) - bias) + beta * C ;  A, C are T ; B is TB (converted on load)
// Extras: C2 = optional second destination; lower_only skips tiles strictly above the diagonal;
// gridDim.z > 1 = split-K (each z-slice accumulates its K range into C with fp64/fp32 atomics; the
// launcher has already applied beta to C).
template <typename T, typename TBs, bool TA, bool TB>
__global__ __launch_bounds__(256) void gemm_kernel(int64_t M, int64_t N, int64_t K, T alpha,
                                                   const T* __restrict__ A, int64_t lda,
                                                   const TBs* __restrict__ B, int64_t ldb, T beta,
                                                   T* __restrict__ C, int64_t ldc,
                                                   const double* __restrict__ bias, T* __restrict__ C2,
                                                   int64_t ldc2, int lower_only, int64_t k_per_split) {
  __shared__ T As[2][GK][GB + GP];
  __shared__ T Bs[2][GK][GB + GP];
  const int tid = threadIdx.x;
  const int lane = tid & 63, wave = tid >> 6;
  const int wr = wave >> 1, wc = wave & 1;
  const int64_t m0 = int64_t(blockIdx.y) * GB, n0 = int64_t(blockIdx.x) * GB;
  if (lower_only && n0 > m0 + (GB - 1)) return;
  const int64_t kz0 = int64_t(blockIdx.z) * k_per_split;
  const int64_t kz1 = min(K, kz0 + k_per_split);
  const bool split = gridDim.z > 1;

  typename Mfma16<T>::acc_t acc[2][2];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int r = 0; r < 4; ++r) acc[i][j][r] = T(0);

  T ra[4], rb[4];
  auto load_regs = [&](int64_t k0) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      int m, k;
      if (TA) { m = tid & 63; k = (tid >> 6) + 4 * i; } else { k = tid & 15; m = (tid >> 4) + 16 * i; }
      const int64_t gm = m0 + m, gk = k0 + k;
      T v = T(0);
      if (gm < M && gk < kz1) v = TA ? A[gk * lda + gm] : A[gm * lda + gk];
      ra[i] = v;
      int n, kb;
      if (TB) { kb = tid & 15; n = (tid >> 4) + 16 * i; } else { n = tid & 63; kb = (tid >> 6) + 4 * i; }
      const int64_t gn = n0 + n, gkb = k0 + kb;
      T w = T(0);
      if (gn < N && gkb < kz1) w = T(TB ? B[gn * ldb + gkb] : B[gkb * ldb + gn]);
      rb[i] = w;
    }
  };
  auto store_regs = [&](int buf) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      int m, k;
      if (TA) { m = tid & 63; k = (tid >> 6) + 4 * i; } else { k = tid & 15; m = (tid >> 4) + 16 * i; }
      As[buf][k][m] = ra[i];
      int n, kb;
      if (TB) { kb = tid & 15; n = (tid >> 4) + 16 * i; } else { n = tid & 63; kb = (tid >> 6) + 4 * i; }
      Bs[buf][kb][n] = rb[i];
    }
  };

  const int64_t nk = (kz1 - kz0 + GK - 1) / GK;
  if (nk <= 0) return;
  load_regs(kz0);
  store_regs(0);
  __syncthreads();
  for (int64_t kt = 0; kt < nk; ++kt) {
    const int cur = int(kt & 1);
    if (kt + 1 < nk) load_regs(kz0 + (kt + 1) * GK);
#pragma unroll
    for (int kk = 0; kk < GK / 4; ++kk) {
      const int kr = 4 * kk + (lane >> 4);
      T a[2], b[2];
#pragma unroll
      for (int t = 0; t < 2; ++t) {
        a[t] = As[cur][kr][wr * 32 + t * 16 + (lane & 15)];
        b[t] = Bs[cur][kr][wc * 32 + t * 16 + (lane & 15)];
      }
#pragma unroll
      for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) acc[i][j] = Mfma16<T>::run(a[i], b[j], acc[i][j]);
    }
    if (kt + 1 < nk) store_regs(cur ^ 1);
    __syncthreads();
  }
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int64_t gm = m0 + wr * 32 + i * 16 + Mfma16<T>::row(lane, r);
        const int64_t gn = n0 + wc * 32 + j * 16 + (lane & 15);
        if (gm < M && gn < N) {
          T v = acc[i][j][r];
          if (bias && blockIdx.z == 0) v -= T(bias[gn]);
          v *= alpha;
          if (split) {
            unsafeAtomicAdd(&C[gm * ldc + gn], v);
          } else {
            if (beta != T(0)) v += beta * C[gm * ldc + gn];
            C[gm * ldc + gn] = v;
            if (C2) C2[gm * ldc2 + gn] = v;
          }
        }
      }
}

template <typename T>
__global__ void k_scale2d(int64_t total, int64_t cols, T* __restrict__ A, int64_t lda, T beta) {
  for (int64_t i = int64_t(blockIdx.x) * blockDim.x + threadIdx.x; i < total; i += int64_t(gridDim.x) * blockDim.x) {
    const int64_t r = i / cols, cc = i - r * cols;
    A[r * lda + cc] = beta == T(0) ? T(0) : beta * A[r * lda + cc];
  }
}

template <typename T, typename TBs>
static void gemm_launch(ccz_ctx* c, bool tA, bool tB, int64_t M, int64_t N, int64_t K, T alpha, const T* A,
                        int64_t lda, const TBs* B, int64_t ldb, T beta, T* C, int64_t ldc, const double* bias,
                        T* C2 = nullptr, int64_t ldc2 = 0, bool lower_only = false) {
  if (M <= 0 || N <= 0) return;
  const int64_t tm = (M + GB - 1) / GB, tn = (N + GB - 1) / GB;
  if (tm > 65535) fail(CCZ_EUNSUP, "gemm: M=%lld too large for one launch", (long long)M);
  hipStream_t st = stream(c);
  // split-K when the output has too few tiles to fill the chip and K is deep (skinny products of the
  // subspace iteration: 4096 x 80 outputs over K = 4096)
  int splits = 1;
  const int ncu = std::max(1, impl(c)->props.multiProcessorCount);
  if (!C2 && !lower_only && tm * tn * 2 <= ncu && K >= 1024) {
    splits = int(std::min<int64_t>({int64_t(32), (2 * ncu) / (tm * tn), K / 256}));
    if (splits < 2) splits = 1;
  }
  int64_t kps = K;
  if (splits > 1) {
    kps = ((K + splits - 1) / splits + GK - 1) / GK * GK;
    splits = int((K + kps - 1) / kps);
    const int64_t total = M * N;
    hipLaunchKernelGGL(k_scale2d<T>, dim3((unsigned)std::min<int64_t>((total + 255) / 256, 1 << 20)), dim3(256), 0, st,
                       total, N, C, ldc, beta);
  }
  dim3 grid((unsigned)tn, (unsigned)tm, (unsigned)splits);
  const int lo = lower_only ? 1 : 0;
  if (!tA && !tB) hipLaunchKernelGGL((gemm_kernel<T, TBs, false, false>), grid, dim3(256), 0, st, M, N, K, alpha, A, lda, B, ldb, beta, C, ldc, bias, C2, ldc2, lo, kps);
  else if (tA && !tB) hipLaunchKernelGGL((gemm_kernel<T, TBs, true, false>), grid, dim3(256), 0, st, M, N, K, alpha, A, lda, B, ldb, beta, C, ldc, bias, C2, ldc2, lo, kps);
  else if (!tA && tB) hipLaunchKernelGGL((gemm_kernel<T, TBs, false, true>), grid, dim3(256), 0, st, M, N, K, alpha, A, lda, B, ldb, beta, C, ldc, bias, C2, ldc2, lo, kps);
  else hipLaunchKernelGGL((gemm_kernel<T, TBs, true, true>), grid, dim3(256), 0, st, M, N, K, alpha, A, lda, B, ldb, beta, C, ldc, bias, C2, ldc2, lo, kps);
  CCZ_LAUNCH_CHECK();
}

void gemm(ccz_ctx* c, bool tA, bool tB, int64_t M, int64_t N, int64_t K, double alpha, const double* A,
          int64_t lda, const double* B, int64_t ldb, double beta, double* C, int64_t ldc) {
  if (gemm_f64_skinny_eligible(tA, tB, M, N, K, A, lda, B, ldb)) {
    gemm_f64_skinny(c, tA, M, N, K, alpha, A, lda, B, ldb, beta, C, ldc);
    return;
  }
  if (gemm_f64_big_eligible(tA, tB, M, N, K, A, lda, B, ldb, C, ldc)) {
    gemm_f64_big(c, tA, tB, M, N, K, alpha, A, lda, B, ldb, beta, C, ldc, false);
    return;
  }
  // split very tall outputs so that grid.y stays legal
  const int64_t maxM = int64_t(65535) * GB;
  for (int64_t m = 0; m < M; m += maxM) {
    const int64_t mm = std::min(maxM, M - m);
    const double* Ap = tA ? A + m : A + m * lda;
    gemm_launch<double, double>(c, tA, tB, mm, N, K, alpha, Ap, lda, B, ldb, beta, C + m * ldc, ldc, nullptr);
  }
}

void gemm_ex(ccz_ctx* c, bool tA, bool tB, int64_t M, int64_t N, int64_t K, double alpha, const double* A,
             int64_t lda, const double* B, int64_t ldb, double beta, double* C, int64_t ldc, double* C2,
             int64_t ldc2, bool lower_only) {
  if (!C2 && !lower_only && gemm_f64_skinny_eligible(tA, tB, M, N, K, A, lda, B, ldb)) {
    gemm_f64_skinny(c, tA, M, N, K, alpha, A, lda, B, ldb, beta, C, ldc);
    return;
  }
  if (!C2 && gemm_f64_big_eligible(tA, tB, M, N, K, A, lda, B, ldb, C, ldc)) {
    gemm_f64_big(c, tA, tB, M, N, K, alpha, A, lda, B, ldb, beta, C, ldc, lower_only);
    return;
  }
  const int64_t maxM = int64_t(65535) * GB;
  if (M > maxM) fail(CCZ_EUNSUP, "gemm_ex: M too large");
  gemm_launch<double, double>(c, tA, tB, M, N, K, alpha, A, lda, B, ldb, beta, C, ldc, nullptr, C2, ldc2, lower_only);
}

void gemm_mixed(ccz_ctx* c, int dtype, int64_t M, int64_t N, int64_t K, double alpha, const void* A, int64_t lda,
                const double* B, int64_t ldb, double beta, void* C, int64_t ldc, const double* bias_row) {
  if (dtype == CCZ_F32 && gemm_f32_big_eligible(M, N, K, lda, ldb, ldc, A, C)) {
    gemm_f32_big(c, M, N, K, alpha, static_cast<const float*>(A), lda, B, ldb, beta, static_cast<float*>(C), ldc, bias_row);
    return;
  }
  const int64_t maxM = int64_t(65535) * GB;
  for (int64_t m = 0; m < M; m += maxM) {
    const int64_t mm = std::min(maxM, M - m);
    if (dtype == CCZ_F32)
      gemm_launch<float, double>(c, false, false, mm, N, K, float(alpha), static_cast<const float*>(A) + m * lda, lda,
                                 B, ldb, float(beta), static_cast<float*>(C) + m * ldc, ldc, bias_row);
    else
      gemm_launch<double, double>(c, false, false, mm, N, K, alpha, static_cast<const double*>(A) + m * lda, lda, B,
                                  ldb, beta, static_cast<double*>(C) + m * ldc, ldc, bias_row);
  }
}

}  // namespace ccz
