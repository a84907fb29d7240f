// Row-sparse reduced-rank regression by ADMM: the coefficient step of CCAR3, whole iterations on the device.
//
// Reference: cca_zoo/linear/_ccar3.py:37-80 (_admm_row_sparse_rrr).  With M = (Sxx + (rho + eps) I)^-1 (p x p, formed once by
// the caller: the reference solves with the Cholesky factor every iteration, the explicit inverse is harmless because the
// matrix's condition number is at most (lambda_max + rho) / rho) and P = Sxy Sy^-1/2 (p x q), from Z = U = 0:
//   B = M (P + rho (Z - U));  Z_old = Z;  Z = B + U with every row scaled by max(0, 1 - (lambda / rho) / |row|) (a zero row
//   stays zero);  U += B - Z;  stop when max(|Z - B|_F, |Z_old - Z|_F) / sqrt(p) < tol, or after max_iter.  The result is Z.
// Limits: p + q <= 16384 (the largest D the moments path has been run at), q <= 1024.
//
// One iteration is two launches, cut at the all-to-all seam (every row of B needs all of rhs):
//   k_rrr_step<NT>      grid (row blocks), 256 threads.  A workgroup owns 16 rows of B and all q columns: its four waves are four
//                       column groups, a wave holds NT = 1, 2, 4, 8 or 16 tiles (16 x 16) of v_mfma_f64_16x16x4f64 (lane maps as
//                       in cp_als.hip: A operand row = lane & 15, k = lane >> 4; B operand k = lane >> 4, column = lane & 15;
//                       C/D column = lane & 15, row = (lane >> 4) + 4 reg).  q <= 4: plain FMAs, 64 rows x 4 columns, one
//                       thread per entry.  Per slab of KC contraction indices it stages its rows of M and KC rows of rhs in
//                       LDS (row, column and contraction tails zero-filled).  A whole row of B lives in one workgroup, so on the
//                       same rows it then forms |B + U| per row (16 lanes by an xor butterfly, the column groups through LDS in
//                       index order), the shrink, its rows of Z and U (in place: nobody else reads them) and of the NEXT
//                       rhs = P + rho (Z - U) into the other of two rhs buffers, so no workgroup reads what another is
//                       writing; and its partial sums of |Z - B|^2 and |Z_old - Z|^2.  Which rhs buffer is current follows
//                       the parity of the iteration count in the status word.
//   k_rrr_finish        one workgroup: the partials folded in index order, the stop test, the count, `stopped`.
// Every kernel reads the status word first and returns at once after the stop.  No floating-point atomics and every sum in a
// fixed order that does not depend on the tiling: two fits give the same bits, whatever the chunk length.
//
// Also here: ccz_rownorm4, the streaming sum_i |y_i - mean|^4 that Ledoit-Wolf's shrinkage needs beside the second moments,
// and ccz_moments_block, a scaled / centred / shifted block of the moments as a dense matrix.
#include <algorithm>
#include <cmath>
#include <cstring>

#include "hip_common.h"
#include "abi_guard.h"
#include "fit_driver.h"
#include "reduce.h"

namespace ccz {

namespace {

constexpr int64_t RRR_MAXD = 16384;                   // p + q
constexpr int RRR_MAXQ = 1024;
constexpr int RRR_PLAIN_Q = 4;                        // q up to which the product runs on plain FMAs
constexpr int RRR_SLAB = 4096;                        // most doubles of one staged rhs slab
constexpr int RRR_FT = 256;                           // threads of k_rrr_finish

constexpr int RRR_RUNNING = 0, RRR_TOL = 1, RRR_MAXITER = 2;   // RrrStatus::reason (include/ccz.h: CCZ_RRR_*)

typedef double v4f64 __attribute__((ext_vector_type(4)));

struct RrrStatus {
  double primal;                   // |Z - B|_F / sqrt(p) of the last finished iteration
  double dual;                     // |Z_old - Z|_F / sqrt(p)
  long long iters;                 // iterations done
  int stopped;
  int reason;
};

struct RrrBuf {
  const double* Minv;              // p x p
  const double* P;                 // p x q
  double* Z;                       // p x q
  double* U;                       // p x q
  double* rhs[2];                  // p x q each: iteration t reads rhs[t & 1] and writes rhs[(t + 1) & 1]
  double* part;                    // 2 per workgroup of k_rrr_step: |Z - B|^2, |Z_old - Z|^2
  int p, q, nblk;
  double thr, rho, tol;            // thr = lambda / rho
  long long max_iter;
};

// Z = U = 0, rhs[0] = P, the status word of a new fit
__global__ void __launch_bounds__(256) k_rrr_start(RrrBuf B, RrrStatus* st) {
  const int64_t total = int64_t(B.p) * B.q;
  for (int64_t e = int64_t(blockIdx.x) * 256 + threadIdx.x; e < total; e += int64_t(gridDim.x) * 256) {
    B.Z[e] = 0.0;
    B.U[e] = 0.0;
    B.rhs[0][e] = B.P[e];
  }
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    st->primal = 0.0; st->dual = 0.0; st->iters = 0; st->stopped = 0; st->reason = RRR_RUNNING;
  }
}

template <int NT>   // 0: plain FMAs (q <= 4); else that many 16-column tiles per wave
__global__ void __launch_bounds__(256) k_rrr_step(RrrBuf B, const RrrStatus* st) {
  if (fit_stopped(st)) return;
  constexpr bool PLAIN = NT == 0;
  constexpr int CW = PLAIN ? 1 : 4;                            // column groups (waves along the columns)
  constexpr int ROWS = PLAIN ? 64 : 16;                        // rows of B per workgroup
  constexpr int QW = PLAIN ? RRR_PLAIN_Q : 16 * CW * NT;       // staged columns
  constexpr int KC = QW <= 128 ? 32 : RRR_SLAB / QW;           // contraction indices per slab
  constexpr int UW = KC + 4;                                   // LDS row stride of the staged rows of M (36 % 32 == 4, as cp_als.hip)
  constexpr int KS = (QW % 32 == 0) ? QW + 16 : QW;            // of the staged rhs rows (KS % 32 == 16: two rows of a half wave on disjoint slots)
  constexpr int NE = PLAIN ? 1 : 4 * NT;                       // entries of B per thread
  constexpr int NR = PLAIN ? 1 : 4;                            // rows per thread
  __shared__ double Ms[ROWS * UW];
  __shared__ double Rs[KC * KS];
  __shared__ double nrm[CW * ROWS];
  __shared__ double red[4];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, li = lane & 15, lg = lane >> 4;
  const int cw = PLAIN ? 0 : wave;
  const int p = B.p, q = B.q;
  const int r0 = int(blockIdx.x) * ROWS;
  const int par = int(st->iters & 1);
  const double* __restrict__ cur = B.rhs[par];
  double* __restrict__ nxt = B.rhs[par ^ 1];
  const double* __restrict__ Mi = B.Minv;

  v4f64 acc[PLAIN ? 1 : NT];
#pragma unroll
  for (int t = 0; t < (PLAIN ? 1 : NT); ++t) acc[t] = v4f64{0.0, 0.0, 0.0, 0.0};
  for (int k0 = 0; k0 < p; k0 += KC) {
    __syncthreads();
    for (int e = tid; e < ROWS * KC; e += 256) {
      const int row = e / KC, kk = e % KC;
      const int a = r0 + row, k = k0 + kk;
      Ms[row * UW + kk] = (a < p && k < p) ? Mi[int64_t(a) * p + k] : 0.0;
    }
    for (int e = tid; e < KC * QW; e += 256) {
      const int kk = e / QW, c = e % QW;
      const int k = k0 + kk;
      Rs[kk * KS + c] = (k < p && c < q) ? cur[int64_t(k) * q + c] : 0.0;
    }
    __syncthreads();
    if constexpr (PLAIN) {
      const int row = tid >> 2, c = tid & 3;
      double s = acc[0][0];
#pragma unroll 8
      for (int kk = 0; kk < KC; ++kk) s += Ms[row * UW + kk] * Rs[kk * KS + c];
      acc[0][0] = s;
    } else {
      const double* ar = Ms + li * UW + lg;
      const double* br = Rs + lg * KS + 16 * cw * NT + li;
#pragma unroll
      for (int k4 = 0; k4 < KC; k4 += 4) {
        const double av = ar[k4];
#pragma unroll
        for (int t = 0; t < NT; ++t) acc[t] = __builtin_amdgcn_mfma_f64_16x16x4f64(av, br[k4 * KS + 16 * t], acc[t], 0, 0, 0);
      }
    }
  }

  // entry e of this thread: local row erow(e), column ecol(e), value acc[e >> 2][e & 3]
  auto erow = [&](int e) { return PLAIN ? (tid >> 2) : lg + 4 * (e & 3); };
  auto ecol = [&](int e) { return PLAIN ? (tid & 3) : 16 * (cw * NT + (e >> 2)) + li; };

  // |B + U|^2 per row
  double ss[NR];
#pragma unroll
  for (int g = 0; g < NR; ++g) ss[g] = 0.0;
#pragma unroll
  for (int e = 0; e < NE; ++e) {
    const int a = r0 + erow(e), c = ecol(e);
    if (a < p && c < q) {
      const double z = acc[e >> 2][e & 3] + B.U[int64_t(a) * q + c];
      ss[e & (NR - 1)] += z * z;
    }
  }
#pragma unroll
  for (int g = 0; g < NR; ++g) {
#pragma unroll
    for (int o = PLAIN ? 2 : 8; o > 0; o >>= 1) ss[g] += __shfl_xor(ss[g], o, 64);
  }
  if constexpr (CW > 1) {
    if (li == 0) {
#pragma unroll
      for (int g = 0; g < NR; ++g) nrm[cw * ROWS + lg + 4 * g] = ss[g];
    }
    __syncthreads();
#pragma unroll
    for (int g = 0; g < NR; ++g) {
      double t = 0.0;
#pragma unroll
      for (int w = 0; w < CW; ++w) t += nrm[w * ROWS + lg + 4 * g];
      ss[g] = t;
    }
  }
  double scale[NR];
#pragma unroll
  for (int g = 0; g < NR; ++g) {
    const double nr = sqrt(ss[g]);
    scale[g] = nr > 0.0 ? fmax(0.0, 1.0 - B.thr / nr) : 0.0;
  }

  // the shrink, Z, U, the next rhs, the residual partials
  double pr = 0.0, du = 0.0;
#pragma unroll
  for (int e = 0; e < NE; ++e) {
    const int a = r0 + erow(e), c = ecol(e);
    if (a < p && c < q) {
      const int64_t at = int64_t(a) * q + c;
      const double b = acc[e >> 2][e & 3];
      const double t = b + B.U[at];
      const double z = t * scale[e & (NR - 1)];
      const double u = t - z;
      const double zo = B.Z[at];
      B.Z[at] = z;
      B.U[at] = u;
      nxt[at] = B.P[at] + B.rho * (z - u);
      pr += (z - b) * (z - b);
      du += (zo - z) * (zo - z);
    }
  }
  pr = block_sum<4>(pr, red);
  du = block_sum<4>(du, red);
  if (tid == 0) {
    B.part[2 * blockIdx.x] = pr;
    B.part[2 * blockIdx.x + 1] = du;
  }
}

__global__ void __launch_bounds__(RRR_FT) k_rrr_finish(RrrBuf B, RrrStatus* st) {
  if (fit_stopped(st)) return;
  __shared__ double red[RRR_FT / 64];
  double pr = 0.0, du = 0.0;
  for (int g = threadIdx.x; g < B.nblk; g += RRR_FT) {
    pr += B.part[2 * g];
    du += B.part[2 * g + 1];
  }
  pr = block_sum<RRR_FT / 64>(pr, red);
  du = block_sum<RRR_FT / 64>(du, red);
  if (threadIdx.x == 0) {
    const double sp = sqrt(double(B.p));
    const double primal = sqrt(pr) / sp, dual = sqrt(du) / sp;
    const long long it = st->iters + 1;
    st->primal = primal;
    st->dual = dual;
    st->iters = it;
    if (fmax(primal, dual) < B.tol) { st->stopped = 1; st->reason = RRR_TOL; }
    else if (it >= B.max_iter) { st->stopped = 1; st->reason = RRR_MAXITER; }
  }
}

// ---- sum_i |y_i - mean|^4 of DEVICE rows --------------------------------------------------------------------------------
// grid (row chunks), 256 threads; a wave takes every fourth row of the chunk, its lanes stride over the columns
template <typename T>
__global__ void __launch_bounds__(256) k_rownorm4(const T* __restrict__ Y, int64_t ld, int cols, int64_t n, int rc,
                                                  const double* __restrict__ mean, double* __restrict__ part) {
  __shared__ double red[4];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int64_t rb = int64_t(blockIdx.x) * rc, re = min(n, rb + rc);
  double s4 = 0.0;
  for (int64_t r = rb + wave; r < re; r += 4) {
    double s = 0.0;
    for (int c = lane; c < cols; c += 64) {
      const double d = double(Y[r * ld + c]) - (mean ? mean[c] : 0.0);
      s += d * d;
    }
    s = wave_sum(s);
    s4 += s * s;
  }
  __syncthreads();
  if (lane == 0) red[wave] = s4;
  __syncthreads();
  if (threadIdx.x == 0) part[blockIdx.x] = ((red[0] + red[1]) + red[2]) + red[3];
}

__global__ void __launch_bounds__(256) k_fold1(const double* __restrict__ part, int count, double* __restrict__ out) {
  __shared__ double red[4];
  double s = 0.0;
  for (int g = threadIdx.x; g < count; g += 256) s += part[g];
  s = block_sum<4>(s, red);
  if (threadIdx.x == 0) *out = s;
}

// ---- host driver ----------------------------------------------------------------------------------------------------
struct RrrState : FitState<RrrStatus> {
  RrrBuf B;
  int nt = 0;                       // the instantiation of k_rrr_step (0: plain)
  bool ready = false;
};

template <int NT>
void launch_step(ccz_ctx* c, const RrrState& S) {
  hipLaunchKernelGGL((k_rrr_step<NT>), dim3(unsigned(S.B.nblk)), dim3(256), 0, stream(c), S.B, S.drv.dev);
}

void enqueue_iteration(ccz_ctx* c, const RrrState& S) {
  switch (S.nt) {
    case 0: launch_step<0>(c, S); break;
    case 1: launch_step<1>(c, S); break;
    case 2: launch_step<2>(c, S); break;
    case 4: launch_step<4>(c, S); break;
    case 8: launch_step<8>(c, S); break;
    default: launch_step<16>(c, S); break;
  }
  CCZ_LAUNCH_CHECK();
  hipLaunchKernelGGL(k_rrr_finish, dim3(1), dim3(RRR_FT), 0, stream(c), S.B, S.drv.dev);
  CCZ_LAUNCH_CHECK();
}

// tiles per wave: the 16-column tiles of q over the four waves, rounded up to a power of two (0: the plain kernel)
int tiles_per_wave(int64_t q) {
  if (q <= RRR_PLAIN_Q) return 0;
  int nt = 1;
  while (int64_t(64) * nt < q) nt *= 2;
  return nt;
}

RrrState* rrr_create(ccz_ctx* c, int64_t p, int64_t q, double lambda, double rho, double tol, int64_t max_iter, int64_t chunk) {
  if (p < 1 || q < 1) fail(CCZ_EINVAL, "rrr: p and q must be at least 1");
  if (p + q > RRR_MAXD) fail(CCZ_EUNSUP, "rrr: p + q = %lld exceeds %lld", (long long)(p + q), (long long)RRR_MAXD);
  if (q > RRR_MAXQ) fail(CCZ_EUNSUP, "rrr: q = %lld exceeds %d (one workgroup holds a whole row of B)", (long long)q, RRR_MAXQ);
  if (!(lambda >= 0.0) || !(rho > 0.0) || !(tol >= 0.0) || !std::isfinite(lambda) || !std::isfinite(rho) || max_iter < 1 || chunk < 1)
    fail(CCZ_EINVAL, "rrr: bad argument");
  return new_state<RrrState>(c, [&](RrrState& S) {
    S.dtype = CCZ_F64; S.M = 2; S.chunk = chunk;
    S.p = {p, q};
    S.nt = tiles_per_wave(q);
    RrrBuf& B = S.B;
    memset(&B, 0, sizeof(B));
    const int rows = S.nt == 0 ? 64 : 16;
    B.p = int(p); B.q = int(q); B.nblk = int((p + rows - 1) / rows);
    B.thr = lambda / rho; B.rho = rho; B.tol = tol; B.max_iter = max_iter;
    const size_t pq = size_t(p) * size_t(q);
    B.Z = S.get(c, pq);
    B.U = S.get(c, pq);
    B.rhs[0] = S.get(c, pq);
    B.rhs[1] = S.get(c, pq);
    B.part = S.get(c, size_t(2) * B.nblk);
    S.drv.create(c);
  });
}

RrrStatus read_status(ccz_ctx* c, const RrrState& S) {
  RrrStatus st;
  d2h(c, &st, S.drv.dev, sizeof(st));
  return st;
}

}  // namespace
}  // namespace ccz

extern "C" {

int ccz_rrr_create(ccz_handle h, int64_t p, int64_t q, double lambda_, double rho, double tol, int64_t max_iter, int64_t chunk_iters,
                   void** state_out) {
  CCZ_GUARD(h, {
    if (!state_out) ccz::fail(CCZ_EINVAL, "null argument");
    *state_out = nullptr;
    *state_out = ccz::rrr_create(h, p, q, lambda_, rho, tol, max_iter, chunk_iters);
  })
}

int ccz_rrr_destroy(ccz_handle h, void* state) {
  CCZ_GUARD(h, {
    if (state) ccz::free_state(h, static_cast<ccz::RrrState*>(state));
  })
}

int ccz_rrr_setup(ccz_handle h, void* state, const double* Minv_dev, const double* P_dev) {
  CCZ_GUARD(h, {
    ccz::RrrState& S = *ccz::as_state<ccz::RrrState>("rrr", state);
    if (!Minv_dev || !P_dev) ccz::fail(CCZ_EINVAL, "rrr: null matrix");
    S.restart(h);
    S.ready = false;
    S.B.Minv = Minv_dev;
    S.B.P = P_dev;
    const int64_t total = int64_t(S.B.p) * S.B.q;
    hipLaunchKernelGGL(ccz::k_rrr_start, dim3(unsigned(std::min<int64_t>((total + 255) / 256, 1024))), dim3(256), 0, ccz::stream(h), S.B,
                       S.drv.dev);
    CCZ_LAUNCH_CHECK();
    S.ready = true;
  })
}

int ccz_rrr_iterations(ccz_handle h, void* state, int64_t n_iters, int64_t* iters_known, int* stopped_known) {
  CCZ_GUARD(h, {
    ccz::RrrState& S = *ccz::as_state<ccz::RrrState>("rrr", state);
    if (!S.ready) ccz::fail(CCZ_EINVAL, "rrr: ccz_rrr_setup has not been called");
    ccz::run_chunk(h, "rrr", "n_iters", S, n_iters, iters_known, stopped_known, &ccz::RrrStatus::iters, [] { return 0; },
                   [&](int, int64_t) { ccz::enqueue_iteration(h, S); });
  })
}

int ccz_rrr_status(ccz_handle h, void* state, int64_t* iters, int* stopped, int* reason, double* primal, double* dual) {
  CCZ_GUARD(h, {
    ccz::RrrState& S = *ccz::as_state<ccz::RrrState>("rrr", state);
    if (!S.ready) ccz::fail(CCZ_EINVAL, "rrr: ccz_rrr_setup has not been called");
    const ccz::RrrStatus st = ccz::read_status(h, S);
    if (iters) *iters = st.iters;
    if (stopped) *stopped = st.stopped;
    if (reason) *reason = st.reason;
    if (primal) *primal = st.primal;
    if (dual) *dual = st.dual;
  })
}

int ccz_rrr_get_result(ccz_handle h, void* state, double* Z_host, double* Z_dev) {
  CCZ_GUARD(h, {
    ccz::RrrState& S = *ccz::as_state<ccz::RrrState>("rrr", state);
    if (!S.ready) ccz::fail(CCZ_EINVAL, "rrr: ccz_rrr_setup has not been called");
    const size_t bytes = size_t(S.B.p) * size_t(S.B.q) * 8;
    if (Z_dev) ccz::d2d(h, Z_dev, S.B.Z, bytes);
    if (Z_host) ccz::d2h(h, Z_host, S.B.Z, bytes);
  })
}

int ccz_rownorm4(ccz_handle h, int dtype, const ccz_view* view, int64_t n_rows, const double* mean_dev, double* out_host) {
  CCZ_GUARD(h, {
    if (!view || !view->data || !out_host || n_rows < 1 || n_rows > (int64_t(1) << 30) || view->cols < 1 || view->cols > ccz::RRR_MAXD ||
        view->ld < view->cols)
      ccz::fail(CCZ_EINVAL, "rownorm4: bad argument");
    ccz::check_dtype("rownorm4", dtype);
    int nchunk, rc;
    ccz::row_chunks(n_rows, 1024, &nchunk, &rc);
    ccz::DBuf part(h, nchunk), out(h, 1);
    ccz::by_dtype(dtype, [&](auto t) {
      using T = decltype(t);
      hipLaunchKernelGGL((ccz::k_rownorm4<T>), dim3(unsigned(nchunk)), dim3(256), 0, ccz::stream(h), static_cast<const T*>(view->data),
                         view->ld, int(view->cols), n_rows, rc, mean_dev, part.get());
    });
    CCZ_LAUNCH_CHECK();
    hipLaunchKernelGGL(ccz::k_fold1, dim3(1), dim3(256), 0, ccz::stream(h), part.get(), nchunk, out.get());
    CCZ_LAUNCH_CHECK();
    ccz::d2h(h, out_host, out, 8);
  })
}

int ccz_moments_block(ccz_handle h, const double* moments_dev, int64_t D, int64_t n_rows, int center, int64_t r0, int64_t rows, int64_t c0,
                      int64_t cols, double shift, double* out_dev, int64_t ldo) {
  CCZ_GUARD(h, {
    if (!moments_dev || !out_dev || D < 1 || n_rows < 1 || r0 < 0 || c0 < 0 || rows < 1 || cols < 1 || r0 + rows > D || c0 + cols > D ||
        ldo < cols)
      ccz::fail(CCZ_EINVAL, "moments_block: bad argument");
    if (shift != 0.0 && (r0 != c0 || rows != cols)) ccz::fail(CCZ_EINVAL, "moments_block: a shift needs a diagonal block");
    ccz::cov_block(h, moments_dev, D, moments_dev + D * D, n_rows, center != 0, 1.0 / double(n_rows), r0, rows, c0, cols, out_dev, ldo);
    if (shift != 0.0) ccz::add_diag(h, rows, out_dev, ldo, shift);
  })
}

}  // extern "C"
