// Kernel matrices of the nonparametric models (KCCA / KGCCA) on the fp64 matrix pipe.
//
//   K[i][j] = f(<a_i - mu, b_j - nu>, ||a_i - mu||^2, ||b_j - nu||^2)          (ccz_pairwise_kernel)
//   out     = K(A, B)' W          without ever writing K                        (ccz_kernel_project)
//
// A and B are fp32 or fp64 rows; mu / nu are optional (centring on load).  Both dtypes go through
// v_mfma_f64_16x16x4f64: fp32 operands are exact in fp64.  The squared row norms come from a prologue pass over
// each side (O(n d), against the O(na nb d) products).  f is scikit-learn's pairwise_kernels with filter_params=True:
//   linear   <a,b>
//   poly     (gamma <a,b> + coef0)^degree        (real exponent: NaN where NumPy gives NaN)
//   rbf      exp(-gamma max(||a||^2 + ||b||^2 - 2 <a,b>, 0)),  distance exactly 0 on the diagonal of K(A, A)
//   sigmoid  tanh(gamma <a,b> + coef0)
//   cosine   <a,b> / (||a|| ||b||),  0 where either row is zero (sklearn's normalize leaves zero rows at zero)
//
// MFMA lane maps (v_mfma_f64_16x16x4f64): A operand (m = lane & 15, k = lane >> 4), B operand (k = lane >> 4,
// n = lane & 15), C/D: col = lane & 15, row = (lane >> 4) + 4 * reg.
//
// k_kernel_matrix: 256 threads, a 64 x 64 tile of K per workgroup, each wave a 32 x 32 quarter (2 x 2 MFMA tiles).
//   Rows of A and B are staged through LDS 32 features at a time, converted to fp64 and centred on the way in.  In
//   the symmetric case (A is B, mu is nu) only tiles on and above the diagonal run and ops' mirror_upper copies
//   the upper triangle down, so K is exactly symmetric.
// k_kernel_project: 256 threads own 64 test rows (wave w: 16 of them) and k-chunk blockIdx.y of 64 columns of W.
//   For every 64-row chunk of training rows the wave forms its 64 x 16 block S of K in four MFMA accumulators,
//   applies f in registers, and feeds S straight into a second MFMA that sums over the training index:
//   out'[c][t] += sum_i W[i][c] S[i][t].  S's accumulator holds rows g + 4 r (g = lane >> 4) in register r, so the
//   k-step r of that second product takes training rows {g + 4 r} -- W is read with the same permutation from LDS
//   and S never moves between lanes.
#include <cmath>

#include "hip_common.h"
#include "abi_guard.h"

namespace ccz {

namespace {

typedef double v4f64 __attribute__((ext_vector_type(4)));

constexpr int KM_T = 64;           // tile edge (rows of A / rows of B per workgroup)
constexpr int KM_KC = 32;          // features per LDS stage
constexpr int KM_LD = KM_KC + 1;   // LDS row stride (doubles)
constexpr int KP_LDW = 65;         // LDS row stride of the staged W chunk (64 columns)

struct KernelParams {
  int kind;
  double gamma, degree, coef0;
};

// the kind is a template parameter: each kernel instance carries one epilogue (all five inlined 16 times in the
// projection kernel's unrolled loop cost ~370 VGPRs)
template <int KIND>
__device__ __forceinline__ double kernel_fn(const KernelParams& p, double dot, double na2, double nb2, bool same_row) {
  if constexpr (KIND == CCZ_KERNEL_LINEAR) {
    return dot;
  } else if constexpr (KIND == CCZ_KERNEL_POLY) {
    return pow(p.gamma * dot + p.coef0, p.degree);
  } else if constexpr (KIND == CCZ_KERNEL_RBF) {
    const double d2 = same_row ? 0.0 : fmax(na2 + nb2 - 2.0 * dot, 0.0);
    return exp(-p.gamma * d2);
  } else if constexpr (KIND == CCZ_KERNEL_SIGMOID) {
    return tanh(p.gamma * dot + p.coef0);
  } else {  // cosine
    const double s = sqrt(na2) * sqrt(nb2);
    return (na2 > 0.0 && nb2 > 0.0) ? dot / s : 0.0;
  }
}

template <typename T>
__device__ __forceinline__ double load_centred(const T* X, int64_t ld, int64_t n, int64_t d, const double* mean, int64_t r,
                                               int64_t col) {
  if (r >= n || col >= d) return 0.0;
  double v = double(X[r * ld + col]);
  if (mean) v -= mean[col];
  return v;
}

// ||x_r - mean||^2, one wave per row
template <typename T>
__global__ void __launch_bounds__(256) k_row_sqnorm(const T* __restrict__ X, int64_t n, int64_t d, int64_t ld,
                                                    const double* __restrict__ mean, double* __restrict__ out) {
  const int lane = threadIdx.x & 63;
  const int64_t r = int64_t(blockIdx.x) * 4 + (threadIdx.x >> 6);
  if (r >= n) return;
  double s = 0.0;
  for (int64_t j = lane; j < d; j += 64) {
    double v = double(X[r * ld + j]);
    if (mean) v -= mean[j];
    s = fma(v, v, s);
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) s += __shfl_xor(s, off);
  if (lane == 0) out[r] = s;
}

// stage rows [r0, r0 + 64) x features [k0, k0 + KM_KC) of X into LDS (fp64, centred; zero outside)
template <typename T>
__device__ __forceinline__ void stage_rows(const T* __restrict__ X, int64_t ld, int64_t n, int64_t d,
                                           const double* __restrict__ mean, int64_t r0, int64_t k0, double* lds) {
#pragma unroll
  for (int e = 0; e < KM_T * KM_KC / 256; ++e) {
    const int idx = threadIdx.x + 256 * e;
    const int row = idx / KM_KC, col = idx % KM_KC;
    lds[row * KM_LD + col] = load_centred(X, ld, n, d, mean, r0 + row, k0 + col);
  }
}

template <typename T, int KIND>
__global__ void __launch_bounds__(256) k_kernel_matrix(const T* __restrict__ A, int64_t na, int64_t lda,
                                                       const double* __restrict__ muA, const T* __restrict__ B, int64_t nb,
                                                       int64_t ldb, const double* __restrict__ muB, int64_t d,
                                                       const double* __restrict__ nrmA, const double* __restrict__ nrmB,
                                                       KernelParams p, int symmetric, double* __restrict__ K, int64_t ldk) {
  if (symmetric && blockIdx.x < blockIdx.y) return;   // strictly below the diagonal: mirrored afterwards
  __shared__ double As[KM_T * KM_LD];
  __shared__ double Bs[KM_T * KM_LD];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int lr = lane & 15, lk = lane >> 4;
  const int wr = w >> 1, wc = w & 1;
  const int64_t i0 = int64_t(blockIdx.y) * KM_T, j0 = int64_t(blockIdx.x) * KM_T;
  v4f64 acc[2][2];
#pragma unroll
  for (int a = 0; a < 2; ++a)
#pragma unroll
    for (int b = 0; b < 2; ++b) acc[a][b] = v4f64{0.0, 0.0, 0.0, 0.0};

  for (int64_t k0 = 0; k0 < d; k0 += KM_KC) {
    stage_rows(A, lda, na, d, muA, i0, k0, As);
    stage_rows(B, ldb, nb, d, muB, j0, k0, Bs);
    __syncthreads();
#pragma unroll
    for (int kk = 0; kk < KM_KC; kk += 4) {
      double a[2], b[2];
#pragma unroll
      for (int t = 0; t < 2; ++t) {
        a[t] = As[(32 * wr + 16 * t + lr) * KM_LD + kk + lk];
        b[t] = Bs[(32 * wc + 16 * t + lr) * KM_LD + kk + lk];
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
    if (j >= nb) continue;
    const double nb2 = nrmB ? nrmB[j] : 0.0;
#pragma unroll
    for (int ta = 0; ta < 2; ++ta) {
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int64_t i = i0 + 32 * wr + 16 * ta + lk + 4 * r;
        if (i >= na) continue;
        const double na2 = nrmA ? nrmA[i] : 0.0;
        K[i * ldk + j] = kernel_fn<KIND>(p, acc[ta][tb][r], na2, nb2, symmetric && i == j);
      }
    }
  }
}

// out (nb x k, ld ldo) = K(A, B)' W,  W (na x k, ld ldw); workgroup: 64 rows of B x 64 columns of W
template <typename T, int KIND>
__global__ void __launch_bounds__(256) k_kernel_project(const T* __restrict__ A, int64_t na, int64_t lda,
                                                        const double* __restrict__ muA, const T* __restrict__ B, int64_t nb,
                                                        int64_t ldb, const double* __restrict__ muB, int64_t d,
                                                        const double* __restrict__ nrmA, const double* __restrict__ nrmB,
                                                        KernelParams p, const double* __restrict__ W, int64_t k, int64_t ldw,
                                                        double* __restrict__ out, int64_t ldo) {
  // the W chunk (64 x 64) reuses the feature stages' space once the chunk's products are done
  __shared__ double lds[2 * KM_T * KM_LD > KM_T * KP_LDW ? 2 * KM_T * KM_LD : KM_T * KP_LDW];
  double* As = lds;                 // training rows
  double* Bs = lds + KM_T * KM_LD;  // test rows
  double* Ws = lds;
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int lr = lane & 15, lk = lane >> 4;
  const int64_t t0 = int64_t(blockIdx.x) * KM_T;
  const int64_t c0 = int64_t(blockIdx.y) * 64;
  const int ntk = int((k - c0 + 15) / 16) < 4 ? int((k - c0 + 15) / 16) : 4;   // live 16-column tiles of this chunk
  const int64_t tcol = t0 + 16 * w + lr;                                        // this lane's test row (S column)
  const double nb2 = (nrmB && tcol < nb) ? nrmB[tcol] : 0.0;
  v4f64 o[4];
#pragma unroll
  for (int t = 0; t < 4; ++t) o[t] = v4f64{0.0, 0.0, 0.0, 0.0};

  for (int64_t i0 = 0; i0 < na; i0 += KM_T) {
    v4f64 s[4];
#pragma unroll
    for (int t = 0; t < 4; ++t) s[t] = v4f64{0.0, 0.0, 0.0, 0.0};
    for (int64_t k0 = 0; k0 < d; k0 += KM_KC) {
      stage_rows(A, lda, na, d, muA, i0, k0, As);
      stage_rows(B, ldb, nb, d, muB, t0, k0, Bs);
      __syncthreads();
#pragma unroll
      for (int kk = 0; kk < KM_KC; kk += 4) {
        const double b = Bs[(16 * w + lr) * KM_LD + kk + lk];
#pragma unroll
        for (int t = 0; t < 4; ++t) {
          const double a = As[(16 * t + lr) * KM_LD + kk + lk];
          s[t] = __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, s[t], 0, 0, 0);
        }
      }
      __syncthreads();
    }
    // W rows [i0, i0 + 64) x columns [c0, c0 + 64) -> LDS (zero outside)
#pragma unroll
    for (int e = 0; e < 16; ++e) {
      const int idx = threadIdx.x + 256 * e;
      const int row = idx >> 6, col = idx & 63;
      const int64_t gi = i0 + row, gc = c0 + col;
      Ws[row * KP_LDW + col] = (gi < na && gc < k) ? W[gi * ldw + gc] : 0.0;
    }
    __syncthreads();
    // epilogue in registers, then out'[c][t] += sum_i W[i][c] S[i][t]  (k-step r: training rows 16 t + g + 4 r)
#pragma unroll
    for (int t = 0; t < 4; ++t) {
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int li = 16 * t + lk + 4 * r;
        const int64_t gi = i0 + li;
        double v = 0.0;
        if (gi < na) v = kernel_fn<KIND>(p, s[t][r], nrmA ? nrmA[gi] : 0.0, nb2, false);
#pragma unroll
        for (int tk = 0; tk < 4; ++tk) {
          if (tk < ntk) {   // wave-uniform
            const double wv = Ws[li * KP_LDW + 16 * tk + lr];
            o[tk] = __builtin_amdgcn_mfma_f64_16x16x4f64(wv, v, o[tk], 0, 0, 0);
          }
        }
      }
    }
    __syncthreads();
  }
  // o[tk]: row = column 16 tk + lk + 4 r of out, col = test row 16 w + lr
  if (tcol < nb) {
#pragma unroll
    for (int tk = 0; tk < 4; ++tk) {
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int64_t gc = c0 + 16 * tk + lk + 4 * r;
        if (tk < ntk && gc < k) out[tcol * ldo + gc] = o[tk][r];
      }
    }
  }
}

void check_kernel_args(int dtype, int kind, int64_t na, int64_t nb, int64_t d, int64_t lda, int64_t ldb) {
  if (dtype != CCZ_F32 && dtype != CCZ_F64) fail(CCZ_EUNSUP, "dtype must be CCZ_F32 or CCZ_F64");
  if (kind < CCZ_KERNEL_LINEAR || kind > CCZ_KERNEL_COSINE) fail(CCZ_EUNSUP, "unknown kernel kind %d", kind);
  if (na < 1 || nb < 1 || d < 1 || lda < d || ldb < d) fail(CCZ_EINVAL, "bad shape");
  if ((na + KM_T - 1) / KM_T > 65535) fail(CCZ_EINVAL, "too many rows (%lld)", (long long)na);
}

template <typename T>
void row_sqnorms(ccz_ctx* c, const void* X, int64_t n, int64_t d, int64_t ld, const double* mean, double* out) {
  hipLaunchKernelGGL(k_row_sqnorm<T>, dim3(unsigned((n + 3) / 4)), dim3(256), 0, stream(c), static_cast<const T*>(X), n, d, ld,
                     mean, out);
  CCZ_LAUNCH_CHECK();
}

bool needs_norms(int kind) { return kind == CCZ_KERNEL_RBF || kind == CCZ_KERNEL_COSINE; }

}  // namespace

void pairwise_kernel(ccz_ctx* c, int dtype, const void* A, int64_t na, int64_t lda, const double* muA, const void* B,
                     int64_t nb, int64_t ldb, const double* muB, int64_t d, int kind, double gamma, double degree,
                     double coef0, double* K, int64_t ldk) {
  check_kernel_args(dtype, kind, na, nb, d, lda, ldb);
  if (!A || !B || !K || ldk < nb) fail(CCZ_EINVAL, "bad argument");
  if ((nb + KM_T - 1) / KM_T > 2147483647LL) fail(CCZ_EINVAL, "too many rows");
  const bool sym = A == B && na == nb && lda == ldb && muA == muB;
  DBuf nrm(c, needs_norms(kind) ? na + (sym ? 0 : nb) : 0);
  double* nA = nrm.get();
  double* nB = nA ? (sym ? nA : nA + na) : nullptr;
  const bool f32 = dtype == CCZ_F32;
  if (nA) {
    (f32 ? row_sqnorms<float> : row_sqnorms<double>)(c, A, na, d, lda, muA, nA);
    if (!sym) (f32 ? row_sqnorms<float> : row_sqnorms<double>)(c, B, nb, d, ldb, muB, nB);
  }
  const KernelParams p{kind, gamma, degree, coef0};
  const dim3 grid(unsigned((nb + KM_T - 1) / KM_T), unsigned((na + KM_T - 1) / KM_T));
  switch (kind) {
#define CCZ_KM_LAUNCH(KIND)                                                                                                 \
  case KIND:                                                                                                                \
    if (f32)                                                                                                                \
      hipLaunchKernelGGL((k_kernel_matrix<float, KIND>), grid, dim3(256), 0, stream(c), static_cast<const float*>(A), na,   \
                         lda, muA, static_cast<const float*>(B), nb, ldb, muB, d, nA, nB, p, sym ? 1 : 0, K, ldk);          \
    else                                                                                                                    \
      hipLaunchKernelGGL((k_kernel_matrix<double, KIND>), grid, dim3(256), 0, stream(c), static_cast<const double*>(A), na, \
                         lda, muA, static_cast<const double*>(B), nb, ldb, muB, d, nA, nB, p, sym ? 1 : 0, K, ldk);         \
    break;
    CCZ_KM_LAUNCH(CCZ_KERNEL_LINEAR)
    CCZ_KM_LAUNCH(CCZ_KERNEL_POLY)
    CCZ_KM_LAUNCH(CCZ_KERNEL_RBF)
    CCZ_KM_LAUNCH(CCZ_KERNEL_SIGMOID)
    CCZ_KM_LAUNCH(CCZ_KERNEL_COSINE)
#undef CCZ_KM_LAUNCH
  }
  CCZ_LAUNCH_CHECK();
  if (sym) mirror_upper(c, na, K, ldk);
}

void kernel_project(ccz_ctx* c, int dtype, const void* A, int64_t na, int64_t lda, const double* muA, const void* B,
                    int64_t nb, int64_t ldb, const double* muB, int64_t d, int kind, double gamma, double degree,
                    double coef0, const double* W, int64_t k, int64_t ldw, double* out, int64_t ldo) {
  check_kernel_args(dtype, kind, na, nb, d, lda, ldb);
  if (!A || !B || !W || !out || k < 1 || ldw < k || ldo < k) fail(CCZ_EINVAL, "bad argument");
  if ((nb + KM_T - 1) / KM_T > 2147483647LL || (k + 63) / 64 > 65535) fail(CCZ_EINVAL, "too many rows or columns");
  DBuf nrm(c, needs_norms(kind) ? na + nb : 0);
  double* nA = nrm.get();
  double* nB = nA ? nA + na : nullptr;
  const bool f32 = dtype == CCZ_F32;
  if (nA) {
    (f32 ? row_sqnorms<float> : row_sqnorms<double>)(c, A, na, d, lda, muA, nA);
    (f32 ? row_sqnorms<float> : row_sqnorms<double>)(c, B, nb, d, ldb, muB, nB);
  }
  const KernelParams p{kind, gamma, degree, coef0};
  const dim3 grid(unsigned((nb + KM_T - 1) / KM_T), unsigned((k + 63) / 64));
  switch (kind) {
#define CCZ_KP_LAUNCH(KIND)                                                                                                  \
  case KIND:                                                                                                                 \
    if (f32)                                                                                                                 \
      hipLaunchKernelGGL((k_kernel_project<float, KIND>), grid, dim3(256), 0, stream(c), static_cast<const float*>(A), na,   \
                         lda, muA, static_cast<const float*>(B), nb, ldb, muB, d, nA, nB, p, W, k, ldw, out, ldo);          \
    else                                                                                                                     \
      hipLaunchKernelGGL((k_kernel_project<double, KIND>), grid, dim3(256), 0, stream(c), static_cast<const double*>(A), na, \
                         lda, muA, static_cast<const double*>(B), nb, ldb, muB, d, nA, nB, p, W, k, ldw, out, ldo);         \
    break;
    CCZ_KP_LAUNCH(CCZ_KERNEL_LINEAR)
    CCZ_KP_LAUNCH(CCZ_KERNEL_POLY)
    CCZ_KP_LAUNCH(CCZ_KERNEL_RBF)
    CCZ_KP_LAUNCH(CCZ_KERNEL_SIGMOID)
    CCZ_KP_LAUNCH(CCZ_KERNEL_COSINE)
#undef CCZ_KP_LAUNCH
  }
  CCZ_LAUNCH_CHECK();
}

}  // namespace ccz


extern "C" {

int ccz_pairwise_kernel(ccz_handle h, int dtype, const void* A_dev, int64_t na, int64_t lda, const double* meanA_dev,
                        const void* B_dev, int64_t nb, int64_t ldb, const double* meanB_dev, int64_t d, int kind,
                        double gamma, double degree, double coef0, double* K_dev, int64_t ldk) {
  CCZ_GUARD(h, ccz::pairwise_kernel(h, dtype, A_dev, na, lda, meanA_dev, B_dev, nb, ldb, meanB_dev, d, kind, gamma, degree,
                                    coef0, K_dev, ldk));
}

int ccz_kernel_project(ccz_handle h, int dtype, const void* A_dev, int64_t na, int64_t lda, const double* meanA_dev,
                       const void* B_dev, int64_t nb, int64_t ldb, const double* meanB_dev, int64_t d, int kind,
                       double gamma, double degree, double coef0, const double* W_dev, int64_t k, int64_t ldw,
                       double* out_dev, int64_t ldo) {
  CCZ_GUARD(h, ccz::kernel_project(h, dtype, A_dev, na, lda, meanA_dev, B_dev, nb, ldb, meanB_dev, d, kind, gamma, degree,
                                   coef0, W_dev, k, ldw, out_dev, ldo));
}

}  // extern "C"
