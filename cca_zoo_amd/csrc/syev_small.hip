// HIP (gfx950 / CDNA4) implementation of the device-op interface in ops.h: jacobi_rows, syev_small.
//
// Float64 dense linear algebra that lives AFTER the Gram reduction: it is latency / launch bound, not on the MFMA
// or HBM roofline (DESIGN.md "solver stage").  The one-workgroup eigen-solvers of the Rayleigh-Ritz steps: one-sided
// Jacobi on rows in LDS, and the two-sided Jacobi for the small symmetric eigenproblems (d <= 160).
#include <algorithm>
#include <cmath>
#include <vector>

#include "hip_common.h"
#include "jacobi_dev.h"

namespace ccz {

// ===========================================================================
// one-sided Jacobi on rows
// ===========================================================================
// Small problems (the Rayleigh-Ritz blocks of the subspace iteration, p ~ 80): the whole W and Q
// live in LDS and ONE workgroup runs every round of every sweep.  A row pair is handled by a
// 16-lane DPP row (64 pairs per pass of the 1024-thread workgroup); the three inner products
// are reduced with DPP lane permutes (quad_perm, row_half_mirror, row_mirror) -- no LDS round
// trips, no launches, no global traffic inside the sweeps.
template <int CTRL>
__device__ __forceinline__ double dpp_mov_f64(double v) {
  const int lo = __builtin_amdgcn_update_dpp(0, __double2loint(v), CTRL, 0xF, 0xF, false);
  const int hi = __builtin_amdgcn_update_dpp(0, __double2hiint(v), CTRL, 0xF, 0xF, false);
  return __hiloint2double(hi, lo);
}
// sum over the 16 lanes of a DPP row, result in every lane of the row
__device__ __forceinline__ double row16_sum(double v) {
  v += dpp_mov_f64<0xB1>(v);    // quad_perm [1,0,3,2]
  v += dpp_mov_f64<0x4E>(v);    // quad_perm [2,3,0,1]
  v += dpp_mov_f64<0x141>(v);   // row_half_mirror
  v += dpp_mov_f64<0x140>(v);   // row_mirror
  return v;
}

__global__ __launch_bounds__(1024) void k_jacobi_lds(int p, int q, double* __restrict__ W, int64_t ldw,
                                                     double* __restrict__ Q, int qc, int64_t ldq, double tol,
                                                     double floor2, int max_sweeps, int* __restrict__ sweeps_out) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int sq = q | 1, sqc = qc | 1;                 // odd row strides: conflict-free column walks
  double* Ws = reinterpret_cast<double*>(smem);
  double* Qs = Ws + size_t(p) * sq;
  // the counter lives at the end of the dynamic region (a static __shared__ object in front of it
  // would shift the region's base off its 16-byte alignment)
  int& rot_count = *reinterpret_cast<int*>(Qs + (Q ? size_t(p) * sqc : 0));
  const int tid = threadIdx.x, gl = tid & 15, grp = tid >> 4, ngrp = blockDim.x >> 4;
  for (int i = tid; i < p * q; i += blockDim.x) Ws[(i / q) * sq + i % q] = W[int64_t(i / q) * ldw + i % q];
  if (Q) for (int i = tid; i < p * qc; i += blockDim.x) Qs[(i / qc) * sqc + i % qc] = Q[int64_t(i / qc) * ldq + i % qc];
  const int pe = (p + 1) & ~1, m1 = pe - 1;
  int sweep = 0, done = 0;
  __syncthreads();
  while (sweep < max_sweeps && !done) {
    ++sweep;
    if (tid == 0) rot_count = 0;
    __syncthreads();
    for (int round = 0; round < m1; ++round) {
      for (int k = grp; k < pe / 2; k += ngrp) {
        int a, b;
        if (k == 0) { a = m1; b = round; } else { a = (round + k) % m1; b = (round - k + m1) % m1; }
        const bool live = a < p && b < p;              // uniform over the 16-lane row
        double* wa = Ws + (live ? a : 0) * sq;
        double* wb = Ws + (live ? b : 0) * sq;
        double al = 0.0, be = 0.0, ga = 0.0;
        if (live)
          for (int t = gl; t < q; t += 16) { const double x = wa[t], y = wb[t]; al += x * x; be += y * y; ga += x * y; }
        al = row16_sum(al); be = row16_sum(be); ga = row16_sum(ga);
        const double prod = al * be;
        if (!live || !(prod > 0.0) || !(fmin(al, be) > floor2) || !(fabs(ga) > tol * sqrt(prod))) continue;
        if (gl == 0) atomicAdd(&rot_count, 1);
        const double zeta = (be - al) / (2.0 * ga);
        const double tt = (zeta >= 0.0 ? 1.0 : -1.0) / (fabs(zeta) + sqrt(1.0 + zeta * zeta));
        const double cs = 1.0 / sqrt(1.0 + tt * tt), sn = cs * tt;
        for (int t = gl; t < q; t += 16) { const double x = wa[t], y = wb[t]; wa[t] = cs * x - sn * y; wb[t] = sn * x + cs * y; }
        if (Q) {
          double* qa = Qs + a * sqc;
          double* qb = Qs + b * sqc;
          for (int t = gl; t < qc; t += 16) { const double x = qa[t], y = qb[t]; qa[t] = cs * x - sn * y; qb[t] = sn * x + cs * y; }
        }
      }
      __syncthreads();
    }
    done = (rot_count == 0);
    __syncthreads();
  }
  for (int i = tid; i < p * q; i += blockDim.x) W[int64_t(i / q) * ldw + i % q] = Ws[(i / q) * sq + i % q];
  if (Q) for (int i = tid; i < p * qc; i += blockDim.x) Q[int64_t(i / qc) * ldq + i % qc] = Qs[(i / qc) * sqc + i % qc];
  if (tid == 0) *sweeps_out = done ? sweep : -1;
}

int jacobi_rows(ccz_ctx* c, int64_t p, int64_t q, double* W, int64_t ldw, double* Q, int64_t qc, int64_t ldq,
                int max_sweeps) {
  if (p < 2) return 1;
  Impl* im = impl(c);
  const size_t lds_need = (size_t(p) * (q | 1) + (Q ? size_t(p) * (qc | 1) : 0)) * 8;
  if (lds_need <= size_t(144) * 1024) {
    const double tol = 2.220446049250313e-16 * std::sqrt(double(q)) * 4.0;
    // rows whose squared norm is below 1e-28 of the largest never rotate (one row_dots + one blocking read-back): only the
    // one-workgroup kernel takes it as an argument -- the block form finds its own on the device
    DBuf nn(c, p);
    row_dots(c, p, q, W, ldw, W, ldw, nn);
    std::vector<double> nh(p);
    d2h(c, nh.data(), nn, size_t(p) * 8);
    double mx = 0.0;
    for (double v : nh) mx = std::max(mx, v);
    const double floor2 = mx * 1e-28;
    CCZ_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(&k_jacobi_lds), hipFuncAttributeMaxDynamicSharedMemorySize, int(lds_need + 16)));
    hipLaunchKernelGGL(k_jacobi_lds, dim3(1), dim3(1024), lds_need + 16, stream(c), int(p), int(q), W, ldw, Q, int(Q ? qc : 0), ldq,
                       tol, floor2, max_sweeps, im->d_flag.get() + 1);
    CCZ_LAUNCH_CHECK();
    int sw = 0;
    d2h(c, &sw, im->d_flag.get() + 1, sizeof(int));
    if (sw < 0) fail(CCZ_ENOCONV, "Jacobi did not converge in %d sweeps (p=%lld, q=%lld)", max_sweeps, (long long)p, (long long)q);
    return sw;
  }
  // evd_block.hip: 32-row blocks, Gram blocks + rotations as MFMA tiles.  It wants a multiple of 64 rows and even
  // leading dimensions (16-byte row pieces): pad with zero rows (they never rotate) when the caller's shape differs.
  const int64_t pp = (p + 63) / 64 * 64;
  if (pp == p && (ldw & 1) == 0 && (!Q || (ldq & 1) == 0)) return jacobi_rows_block(c, p, q, W, ldw, Q, qc, ldq, max_sweeps);
  const int64_t lw = (q + 1) & ~int64_t(1), lq = (qc + 1) & ~int64_t(1);
  DBuf Wp(c, pp * lw), Qp(c, Q ? pp * lq : 0);
  fill2d(c, pp, lw, Wp, lw, 0.0);
  copy2d(c, p, q, W, ldw, Wp, lw);
  if (Q) { fill2d(c, pp, lq, Qp, lq, 0.0); copy2d(c, p, qc, Q, ldq, Qp, lq); }
  const int sw = jacobi_rows_block(c, pp, q, Wp, lw, Q ? Qp.get() : nullptr, qc, lq, max_sweeps);
  copy2d(c, p, q, Wp, lw, W, ldw);
  if (Q) copy2d(c, p, qc, Qp, lq, Q, ldq);
  return sw;
}

// ===========================================================================
// Two-sided (classical) Jacobi for the small symmetric eigenproblems of the Rayleigh-Ritz steps (d <= 96)
// ===========================================================================
// The one-sided kernel above spends a round on three length-d inner products per row pair before it can rotate;
// on a symmetric H the rotation of pair (p, q) follows from h_pp, h_qq, h_pq alone, and one round of the tournament
// (d/2 disjoint pairs) is   H <- J' H J,  V' <- J' V'   with J = product of the round's rotations: every 2 x 2 block
// (row pair a, column pair b) becomes R_a' M R_b independently of all others.  One workgroup, H and V' in LDS, a
// two-stage pipeline per round (parameters double-buffered):
//   A: all 16 waves apply round g to H                                                  | barrier
//   B: wave 0 derives the parameters of round g + 1 from the new H  ||  waves 1..15 apply round g to V'   | barrier
// Every thread owns the same blocks / V' items in every round and gets the round's row indices by two integer
// adds (the tournament shifts positions by one per round): no index tables, no divisions inside the loop, one level
// of LDS latency per stage.  The long-latency part of a round is wave 0's (sqrt, divide, reciprocal sqrt) chain: done
// with v_rsq / v_rcp seeds and two Newton steps each (~200 cycles instead of ~550 for the IEEE expansions).
// Stopping: a sweep without a rotation; a pair is rotated when |h_pq| > tol * max|H| (absolute: the Rayleigh-Ritz
// matrices are indefinite, zero diagonals happen -- MCCA with two views has exact +lam / -lam pairs).
// Rows/columns are padded to an even count; the pad row/column is zero and stays zero (its pair never rotates).
template <int NB_, int NV_>   // H blocks / V' items per thread (compile-time: the slot arrays must stay in registers)
__device__ __forceinline__ void syev_small_body(char* smem, int d, const double* __restrict__ A, int64_t lda, double* __restrict__ w,
                                                double* __restrict__ Vt, int64_t ldv, double tol, int max_sweeps,
                                                int* __restrict__ status) {
  const int pe = (d + 1) & ~1, m1 = pe - 1, np = pe >> 1, sd = pe | 1;
  double* Hs = reinterpret_cast<double*>(smem);
  double* Vs = Hs + pe * sd;
  double* red = Vs + pe * sd;                              // 16 wave maxima
  int* rot = reinterpret_cast<int*>(red + 16);             // [2]: rotations of the even / odd sweeps (+ 2 ints of padding)
  jac_cs* csn = reinterpret_cast<jac_cs*>(red + 18);       // [2][np] (cosine, sine), 16-byte aligned: (2 pe sd + 18) is even
  const int tid = threadIdx.x, nt = blockDim.x;            // nt == 1024
  double mx = 0.0;
  for (int i = tid; i < pe * pe; i += nt) {
    const int r = i / pe, c = i - r * pe;
    double h = 0.0;
    if (r < d && c < d) {
      h = 0.5 * (A[int64_t(r) * lda + c] + A[int64_t(c) * lda + r]);
      const double a = fabs(h);
      mx = (a <= 1.79769313486231570e308) ? fmax(mx, a) : __builtin_inf();   // NaN / inf poison the maximum
    }
    Hs[r * sd + c] = h;
    Vs[r * sd + c] = (r == c && r < d) ? 1.0 : 0.0;
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) mx = fmax(mx, __shfl_xor(mx, o, 64));
  if ((tid & 63) == 0) red[tid >> 6] = mx;
  if (tid < 2) rot[tid] = 0;
  __syncthreads();
  double hmax = 0.0;
  for (int i = 0; i < (nt + 63) >> 6; ++i) hmax = fmax(hmax, red[i]);
  if (!(hmax < __builtin_inf())) {
    if (tid == 0) *status = -2;
    return;
  }
  if (hmax == 0.0) {                                       // the zero matrix: eigenvalues 0, V = I
    for (int i = tid; i < d; i += nt) w[i] = 0.0;
    for (int i = tid; i < d * d; i += nt) Vt[int64_t(i / d) * ldv + i % d] = (i / d == i % d) ? 1.0 : 0.0;
    if (tid == 0) *status = 1;
    return;
  }
  const double thr = tol * hmax, ih = 1.0 / hmax;

  // This thread's blocks of H and items of V': the same in every round.  np <= 48: at most 2304 blocks (3 per
  // thread) and 48 * 96 = 4608 V' items on the 960 threads of waves 1..15 (5 per thread; d <= 80: 2 and 4).  Slots past the end are
  // pointed at block / item 0 and masked at the store, so that every load below is unconditional.
  const int nblk = np * np, nitem = np * d;
  int bka[NB_], bkb[NB_];
  bool bon[NB_];
#pragma unroll
  for (int j = 0; j < NB_; ++j) {
    const int b = tid + j * nt;
    bon[j] = b < nblk;
    bka[j] = bon[j] ? b / np : 0;
    bkb[j] = bon[j] ? b - bka[j] * np : 0;
  }
  const int vt = tid - 64, nvt = nt - 64;                  // waves 1..15 rotate V'
  int vk[NV_], vr[NV_];
  bool von[NV_];
#pragma unroll
  for (int j = 0; j < NV_; ++j) {
    const int it = vt + j * nvt;
    von[j] = vt >= 0 && it < nitem;
    vk[j] = von[j] ? it / d : 0;
    vr[j] = von[j] ? it - vk[j] * d : 0;
  }

  auto params = [&](int round, int buf, int sweep_parity) {              // lanes < np of wave 0
    const int k = tid;
    int a, b;
    pair_of(round, k, m1, a, b);
    const double hpq = Hs[a * sd + b], hqq = Hs[b * sd + b], hpp = Hs[a * sd + a];
    jac_cs r = {1.0, 0.0};
    if (fabs(hpq) > thr) {
      r = jac_rotation(hpp, hqq, hpq, ih);
      atomicAdd(rot + sweep_parity, 1);
    }
    csn[buf * np + k] = r;
  };

  if (tid < np) params(0, 0, 1);                           // sweep 1 is odd
  __syncthreads();
  int sweep = 0, g = 0;
  bool done = false;
  while (sweep < max_sweeps && !done) {
    ++sweep;
    const int par = sweep & 1;
    if (tid == 0) rot[par ^ 1] = 0;                        // next sweep's counter: first incremented in this sweep's last stage B
    for (int round = 0; round < m1; ++round, ++g) {
      const jac_cs* cur = csn + (g & 1) * np;
      // ---- stage A: H <- J' H J, this thread's 2 x 2 blocks; all loads first (one level of LDS latency) ----
      {
        int o[NB_][4];
        double m[NB_][4];
        jac_cs ra[NB_], rb[NB_];
#pragma unroll
        for (int j = 0; j < NB_; ++j) {
            int p1, q1, p2, q2;
            pair_of(round, bka[j], m1, p1, q1);
            pair_of(round, bkb[j], m1, p2, q2);
            o[j][0] = p1 * sd + p2;
            o[j][1] = p1 * sd + q2;
            o[j][2] = q1 * sd + p2;
            o[j][3] = q1 * sd + q2;
            ra[j] = cur[bka[j]];
            rb[j] = cur[bkb[j]];
#pragma unroll
            for (int e = 0; e < 4; ++e) m[j][e] = Hs[o[j][e]];
          }
#pragma unroll
        for (int j = 0; j < NB_; ++j) {
            const double ca = ra[j].x, sa = ra[j].y, cb = rb[j].x, sb = rb[j].y;
            const double n00 = cb * m[j][0] - sb * m[j][1], n01 = sb * m[j][0] + cb * m[j][1];
            const double n10 = cb * m[j][2] - sb * m[j][3], n11 = sb * m[j][2] + cb * m[j][3];
            double o00 = ca * n00 - sa * n10, o10 = sa * n00 + ca * n10;
            double o01 = ca * n01 - sa * n11, o11 = sa * n01 + ca * n11;
            if (bka[j] == bkb[j] && sa != 0.0) { o01 = 0.0; o10 = 0.0; }   // the rotated pair itself: annihilated by construction
            if (bon[j]) { Hs[o[j][0]] = o00; Hs[o[j][1]] = o01; Hs[o[j][2]] = o10; Hs[o[j][3]] = o11; }
          }
      }
      __syncthreads();
      // ---- stage B: wave 0 prepares round g + 1 from the new H; the other waves rotate the rows of V' ----
      if (tid < 64) {
        if (tid < np) {
          const bool last = round + 1 == m1;
          params(last ? 0 : round + 1, (g & 1) ^ 1, last ? (par ^ 1) : par);
        }
      } else {
        int op[NV_], oq[NV_];
        double x[NV_], y[NV_];
        jac_cs r[NV_];
#pragma unroll
        for (int j = 0; j < NV_; ++j) {
            int p, q;
            pair_of(round, vk[j], m1, p, q);
            op[j] = p * sd + vr[j];
            oq[j] = q * sd + vr[j];
            r[j] = cur[vk[j]];
            x[j] = Vs[op[j]];
            y[j] = Vs[oq[j]];
          }
#pragma unroll
        for (int j = 0; j < NV_; ++j)
          if (von[j]) { Vs[op[j]] = r[j].x * x[j] - r[j].y * y[j]; Vs[oq[j]] = r[j].y * x[j] + r[j].x * y[j]; }
      }
      __syncthreads();
    }
    done = (rot[par] == 0);
    __syncthreads();                                       // everyone has read the counter before thread 0 recycles it
  }
  for (int i = tid; i < d; i += nt) w[i] = Hs[i * sd + i];
  for (int i = tid; i < d * d; i += nt) {
    const int r = i / d, c = i - r * d;
    Vt[int64_t(r) * ldv + c] = Vs[r * sd + c];
  }
  if (tid == 0) *status = done ? sweep : -1;
}

__global__ __launch_bounds__(1024) void k_syev_small(int d, const double* __restrict__ A, int64_t lda, double* __restrict__ w,
                                                     double* __restrict__ Vt, int64_t ldv, double tol, int max_sweeps,
                                                     int* __restrict__ status) {
  extern __shared__ __attribute__((aligned(16))) char jac_smem[];
  syev_small_body<2, 4>(jac_smem, d, A, lda, w, Vt, ldv, tol, max_sweeps, status);      // d <= 80
}
__global__ __launch_bounds__(1024) void k_syev_small_wide(int d, const double* __restrict__ A, int64_t lda, double* __restrict__ w,
                                                          double* __restrict__ Vt, int64_t ldv, double tol, int max_sweeps,
                                                          int* __restrict__ status) {
  extern __shared__ __attribute__((aligned(16))) char jac_smem[];
  syev_small_body<3, 5>(jac_smem, d, A, lda, w, Vt, ldv, tol, max_sweeps, status);      // 80 < d <= 96
}

// ---------------------------------------------------------------------------
// The same eigen-solve split in two (default; d <= 160): the fused kernel above moves 306 KB through the LDS of ONE
// CU per round (H and V', each read + written, plus the rotation parameters) and is bound by exactly that.
//   k_syev_packed   one workgroup: H only, stored as its packed lower triangle (the mirrored 2 x 2 blocks are the same
//                   numbers: half the blocks, a quarter of the LDS bytes per round; 103 KB hold d = 160, which the
//                   square layout could not), every round's (c, s) pairs are logged to global memory;
//   k_jacobi_replay d / 16 workgroups: each replays the whole log on its own 16 columns of V' = I (columns of V' are
//                   independent), one barrier per round, parameters of the next round prefetched.
// ---------------------------------------------------------------------------
// Workgroup barrier that orders LDS traffic only.  __syncthreads() is a workgroup-scope fence over ALL address spaces:
// with a global store in flight (the rotation log) every wave would wait for its acknowledgement (~1 us) at every
// barrier of the round loop.  The log is consumed by a later kernel, so only this wave's LDS operations must have
// completed before the barrier.
// sync (may be null): two agent-scope words for the replaying workgroups of the SAME launch (k_syev_chase below) --
//   sync[0] = rounds whose parameters are complete in the log (moved every JR_CHUNK rounds), sync[1] = 1 + rounds to replay once the
//   solve has ended (any way it ends).  The log is stored write-through (st_shared2) so that another XCD's workgroup can read it.
constexpr int JR_CHUNK = 16;                                  // rounds of parameters staged through LDS at a time
template <int NB_>
__device__ __forceinline__ void syev_packed_body(char* smem, int d, const double* __restrict__ A, int64_t lda, double* __restrict__ w,
                                                 jac_cs* __restrict__ log, double tol, int max_sweeps, int* __restrict__ status,
                                                 unsigned* __restrict__ sync = nullptr) {
  const int pe = (d + 1) & ~1, m1 = pe - 1, np = pe >> 1;
  const int nH = pe * (pe + 1) / 2, nHp = (nH + 1) & ~1;
  double* Hs = reinterpret_cast<double*>(smem);
  double* red = Hs + nHp;
  int* rot = reinterpret_cast<int*>(red + 16);
  jac_cs* csn = reinterpret_cast<jac_cs*>(red + 18);       // [2][np]
  const int tid = threadIdx.x, nt = blockDim.x;
  double mx = 0.0;
  for (int e = tid; e < nH; e += nt) {
    int i, j;
    tri_decode(e, i, j);
    double h = 0.0;
    if (i < d) {                                           // j <= i
      h = 0.5 * (A[int64_t(i) * lda + j] + A[int64_t(j) * lda + i]);
      const double a = fabs(h);
      mx = (a <= 1.79769313486231570e308) ? fmax(mx, a) : __builtin_inf();
    }
    Hs[e] = h;
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) mx = fmax(mx, __shfl_xor(mx, o, 64));
  if ((tid & 63) == 0) red[tid >> 6] = mx;
  if (tid < 2) rot[tid] = 0;
  __syncthreads();
  double hmax = 0.0;
  for (int i = 0; i < (nt + 63) >> 6; ++i) hmax = fmax(hmax, red[i]);
  if (!(hmax < __builtin_inf())) {
    if (tid == 0) {
      status[0] = -2; status[1] = 0;
      if (sync) __hip_atomic_store((gu32_ptr)(reinterpret_cast<uintptr_t>(sync + 1)), 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    return;
  }
  if (hmax == 0.0) {
    for (int i = tid; i < d; i += nt) w[i] = 0.0;
    if (tid == 0) {
      status[0] = 1; status[1] = 0;
      if (sync) __hip_atomic_store((gu32_ptr)(reinterpret_cast<uintptr_t>(sync + 1)), 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    return;
  }
  const double thr = tol * hmax, ih = 1.0 / hmax;
  const int nblk = np * (np + 1) / 2;
  int bka[NB_], bkb[NB_];
  bool bon[NB_];
#pragma unroll
  for (int j = 0; j < NB_; ++j) {
    const int b = tid + j * nt;
    bon[j] = b < nblk;
    bka[j] = 0; bkb[j] = 0;
    if (bon[j]) tri_decode(b, bka[j], bkb[j]);            // ka >= kb
  }
  auto params = [&](int round, int buf, int sweep_parity, int glog) {   // lanes < np of wave 0
    const int k = tid;
    int a, b;
    pair_of(round, k, m1, a, b);
    const double hpq = Hs[tri_off(a, b)], hqq = Hs[tri_off(b, b)], hpp = Hs[tri_off(a, a)];
    jac_cs r = {1.0, 0.0};
    if (fabs(hpq) > thr) {
      r = jac_rotation(hpp, hqq, hpq, ih);
      atomicAdd(rot + sweep_parity, 1);
    }
    csn[buf * np + k] = r;
    st_shared2(reinterpret_cast<double*>(log + int64_t(glog) * np + k), r.x, r.y);
  };
  if (tid < np) params(0, 0, 1, 0);
  __syncthreads();
  int sweep = 0, g = 0;
  bool done = false;
  while (sweep < max_sweeps && !done) {
    ++sweep;
    const int par = sweep & 1;
    if (tid == 0) rot[par ^ 1] = 0;
    for (int round = 0; round < m1; ++round, ++g) {
      const jac_cs* cur = csn + (g & 1) * np;
      {
        int o[NB_][4];
        double m[NB_][4];
        jac_cs ra[NB_], rb[NB_];
#pragma unroll
        for (int j = 0; j < NB_; ++j) {
          int p1, q1, p2, q2;
          pair_of(round, bka[j], m1, p1, q1);
          pair_of(round, bkb[j], m1, p2, q2);
          o[j][0] = tri_off(p1, p2);
          o[j][1] = tri_off(p1, q2);
          o[j][2] = tri_off(q1, p2);
          o[j][3] = tri_off(q1, q2);
          ra[j] = cur[bka[j]];
          rb[j] = cur[bkb[j]];
#pragma unroll
          for (int e = 0; e < 4; ++e) m[j][e] = Hs[o[j][e]];
        }
#pragma unroll
        for (int j = 0; j < NB_; ++j) {
          const double ca = ra[j].x, sa = ra[j].y, cb = rb[j].x, sb = rb[j].y;
          const double n00 = cb * m[j][0] - sb * m[j][1], n01 = sb * m[j][0] + cb * m[j][1];
          const double n10 = cb * m[j][2] - sb * m[j][3], n11 = sb * m[j][2] + cb * m[j][3];
          double o00 = ca * n00 - sa * n10, o10 = sa * n00 + ca * n10;
          double o01 = ca * n01 - sa * n11, o11 = sa * n01 + ca * n11;
          if (bka[j] == bkb[j] && sa != 0.0) { o01 = 0.0; o10 = 0.0; }   // the rotated pair itself (one storage cell)
          if (bon[j]) { Hs[o[j][0]] = o00; Hs[o[j][1]] = o01; Hs[o[j][2]] = o10; Hs[o[j][3]] = o11; }
        }
      }
      lds_barrier();
      const bool publish = sync && ((g + 2) & (JR_CHUNK - 1)) == 0;      // rounds 0 .. g + 1 are in the log after this step
      if (tid < np) {
        const bool last = round + 1 == m1;
        params(last ? 0 : round + 1, (g & 1) ^ 1, last ? (par ^ 1) : par, g + 1);
        if (publish) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");      // (the writing lanes drain their write-through stores)
      }
      lds_barrier();
      if (publish && tid == 0)
        __hip_atomic_store((gu32_ptr)(reinterpret_cast<uintptr_t>(sync)), unsigned(g + 2), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    done = (rot[par] == 0);
    lds_barrier();
  }
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
  for (int i = tid; i < d; i += nt) w[i] = Hs[tri_off(i, i)];
  if (tid == 0) {
    status[0] = done ? sweep : -1; status[1] = g;
    // the last sweep of a converged run rotated nothing: the log's first (sweeps - 1) * m1 rounds are all of V
    if (sync) __hip_atomic_store((gu32_ptr)(reinterpret_cast<uintptr_t>(sync + 1)), 1u + unsigned(done ? (sweep - 1) * m1 : 0), __ATOMIC_RELAXED,
                                 __HIP_MEMORY_SCOPE_AGENT);
  }
}

__global__ __launch_bounds__(1024) void k_syev_packed1(int d, const double* __restrict__ A, int64_t lda, double* __restrict__ w,
                                                       jac_cs* __restrict__ log, double tol, int max_sweeps, int* __restrict__ status) {
  extern __shared__ __attribute__((aligned(16))) char jac_smem[];
  syev_packed_body<1>(jac_smem, d, A, lda, w, log, tol, max_sweeps, status);            // d <= 88 (990 blocks)
}
__global__ __launch_bounds__(1024) void k_syev_packed2(int d, const double* __restrict__ A, int64_t lda, double* __restrict__ w,
                                                       jac_cs* __restrict__ log, double tol, int max_sweeps, int* __restrict__ status) {
  extern __shared__ __attribute__((aligned(16))) char jac_smem[];
  syev_packed_body<2>(jac_smem, d, A, lda, w, log, tol, max_sweeps, status);            // d <= 126
}
__global__ __launch_bounds__(1024) void k_syev_packed4(int d, const double* __restrict__ A, int64_t lda, double* __restrict__ w,
                                                       jac_cs* __restrict__ log, double tol, int max_sweeps, int* __restrict__ status) {
  extern __shared__ __attribute__((aligned(16))) char jac_smem[];
  syev_packed_body<4>(jac_smem, d, A, lda, w, log, tol, max_sweeps, status);            // d <= 160 (3240 blocks)
}

constexpr int JR_COLS = 16, JR_SLOTS = 16, JR_MAXK = 5;      // 256 threads: 16 columns x 16 pair slots, np <= 80
__global__ __launch_bounds__(256) void k_jacobi_replay(int d, const jac_cs* __restrict__ log, int rounds, double* __restrict__ Vt,
                                                       int64_t ldv) {
  __shared__ double Vs[160 * (JR_COLS + 1)];
  __shared__ jac_cs Ps[2][JR_CHUNK * 80];                     // two chunks of (c, s): one in use, one being filled
  const int pe = (d + 1) & ~1, m1 = pe - 1, np = pe >> 1;
  const int tid = threadIdx.x, col = tid & (JR_COLS - 1), slot = tid >> 4;
  const int col0 = blockIdx.x * JR_COLS;
  for (int e = tid; e < pe * JR_COLS; e += 256) {
    const int r = e >> 4, cc = e & 15;
    Vs[r * (JR_COLS + 1) + cc] = (r == col0 + cc && r < d) ? 1.0 : 0.0;
  }
  // the log is one contiguous array of rounds * np entries: a chunk is JR_CHUNK * np consecutive entries (<= 1280: 5 per thread)
  const int per_chunk = JR_CHUNK * np;
  const int64_t total = int64_t(rounds) * np;
  jac_cs stage[JR_MAXK];
  auto fetch = [&](int chunk) {
#pragma unroll
    for (int j = 0; j < JR_MAXK; ++j) {
      const int e = tid + 256 * j;
      const int64_t gidx = int64_t(chunk) * per_chunk + e;
      stage[j] = (e < per_chunk && gidx < total) ? log[gidx] : jac_cs{1.0, 0.0};
    }
  };
  auto stash = [&](int buf) {
#pragma unroll
    for (int j = 0; j < JR_MAXK; ++j) {
      const int e = tid + 256 * j;
      if (e < per_chunk) Ps[buf][e] = stage[j];
    }
  };
  const int nchunks = (rounds + JR_CHUNK - 1) / JR_CHUNK;
  if (nchunks > 0) { fetch(0); stash(0); }
  __syncthreads();
  int round = 0;
  for (int ch = 0; ch < nchunks; ++ch) {
    if (ch + 1 < nchunks) fetch(ch + 1);                       // global latency hides behind this chunk's rounds
    const jac_cs* P = Ps[ch & 1];
    const int r_end = min(JR_CHUNK, rounds - ch * JR_CHUNK);
    for (int rr = 0; rr < r_end; ++rr) {
      int op[JR_MAXK], oq[JR_MAXK];
      double x[JR_MAXK], y[JR_MAXK];
      jac_cs cs[JR_MAXK];
#pragma unroll
      for (int j = 0; j < JR_MAXK; ++j) {
        const int k = min(slot + JR_SLOTS * j, np - 1);
        int p, q;
        pair_of(round, k, m1, p, q);
        op[j] = p * (JR_COLS + 1) + col;
        oq[j] = q * (JR_COLS + 1) + col;
        cs[j] = P[rr * np + k];
        x[j] = Vs[op[j]];
        y[j] = Vs[oq[j]];
      }
#pragma unroll
      for (int j = 0; j < JR_MAXK; ++j)
        if (slot + JR_SLOTS * j < np) {
          Vs[op[j]] = cs[j].x * x[j] - cs[j].y * y[j];
          Vs[oq[j]] = cs[j].y * x[j] + cs[j].x * y[j];
        }
      lds_barrier();
      if (++round == m1) round = 0;
    }
    if (ch + 1 < nchunks) stash((ch + 1) & 1);                 // nobody reads that buffer during this chunk
    __syncthreads();
  }
  if (col0 + col < d)
    for (int r = slot; r < d; r += JR_SLOTS) Vt[int64_t(r) * ldv + col0 + col] = Vs[r * (JR_COLS + 1) + col];
}

// ---------------------------------------------------------------------------
// Round 6: eigen-solve and replay as ONE launch (k_syev_chase).  The replay above starts when the solve has ended (and after a host
// round trip for the sweep count): 367 + 294 us behind the 800 + 661 us of the two Rayleigh-Ritz solves of an rCCA fit.  A round of
// the replay takes half the time of a round of the solve, so here the replaying workgroups run NEXT to the solving one and chase
// its log chunk by chunk: workgroup 0 = syev_packed_body (log stored write-through, a progress word every 16 rounds), workgroups
// 1 .. d / 16 = the replay on 16 columns of V' each (their first 256 threads; the rest retire at once), polling the progress word
// and reading the log past their XCD's L2 (ld_shared).  V' is complete one chunk (~15 us) after the solve.  Every exit of the
// solving workgroup publishes the end word; a poller that sees nothing for ~2 s gives up and reports -3.
// ---------------------------------------------------------------------------
constexpr int SC_WATCHDOG = 1 << 24;
__device__ __forceinline__ void replay_chase_body(char* smem, int d, const jac_cs* __restrict__ log, unsigned* __restrict__ sync,
                                                  double* __restrict__ Vt, int64_t ldv, int blk, int* __restrict__ status) {
  double* Vs = reinterpret_cast<double*>(smem);                                  // [pe][JR_COLS + 1]
  jac_cs* Ps = reinterpret_cast<jac_cs*>(Vs + 160 * (JR_COLS + 1));             // one chunk of (c, s)
  int* ctl = reinterpret_cast<int*>(Ps + JR_CHUNK * 80);                         // [0] rounds of this chunk, [1] 1 = last chunk, 2 = gave up
  const int pe = (d + 1) & ~1, m1 = pe - 1, np = pe >> 1;
  const int tid = threadIdx.x, col = tid & (JR_COLS - 1), slot = tid >> 4;
  const int col0 = blk * JR_COLS;
  for (int e = tid; e < pe * JR_COLS; e += 256) {
    const int r = e >> 4, cc = e & 15;
    Vs[r * (JR_COLS + 1) + cc] = (r == col0 + cc && r < d) ? 1.0 : 0.0;
  }
  const gu32_ptr wP = (gu32_ptr)(reinterpret_cast<uintptr_t>(sync)), wF = (gu32_ptr)(reinterpret_cast<uintptr_t>(sync + 1));
  int round = 0;
  bool gave_up = false;
  for (int ch = 0;; ++ch) {
    const int base = ch * JR_CHUNK;
    if (tid == 0) {
      int n = 0, last = 0, spins = 0;
      for (;;) {
        const unsigned F = __hip_atomic_load(wF, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (F != 0u) {
          const int fin = int(F - 1u);
          n = max(0, min(JR_CHUNK, fin - base));
          last = base + JR_CHUNK >= fin ? 1 : 0;
          break;
        }
        if (int(__hip_atomic_load(wP, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) >= base + JR_CHUNK) { n = JR_CHUNK; break; }
        __builtin_amdgcn_s_sleep(8);
        if (++spins > SC_WATCHDOG) { n = 0; last = 2; break; }
      }
      ctl[0] = n;
      ctl[1] = last;
    }
    __syncthreads();
    const int n = ctl[0], last = ctl[1];
    for (int e = tid; e < n * np; e += 256) {
      const double* src = reinterpret_cast<const double*>(log + int64_t(base) * np + e);
      jac_cs r;
      r.x = ld_shared(src);
      r.y = ld_shared(src + 1);
      Ps[e] = r;
    }
    __syncthreads();
    for (int rr = 0; rr < n; ++rr) {
      int op[JR_MAXK], oq[JR_MAXK];
      double x[JR_MAXK], y[JR_MAXK];
      jac_cs cs[JR_MAXK];
#pragma unroll
      for (int j = 0; j < JR_MAXK; ++j) {
        const int k = min(slot + JR_SLOTS * j, np - 1);
        int p, q;
        pair_of(round, k, m1, p, q);
        op[j] = p * (JR_COLS + 1) + col;
        oq[j] = q * (JR_COLS + 1) + col;
        cs[j] = Ps[rr * np + k];
        x[j] = Vs[op[j]];
        y[j] = Vs[oq[j]];
      }
#pragma unroll
      for (int j = 0; j < JR_MAXK; ++j)
        if (slot + JR_SLOTS * j < np) {
          Vs[op[j]] = cs[j].x * x[j] - cs[j].y * y[j];
          Vs[oq[j]] = cs[j].y * x[j] + cs[j].x * y[j];
        }
      lds_barrier();
      if (++round == m1) round = 0;
    }
    __syncthreads();                                           // (ctl and Ps are rewritten by the next chunk)
    if (last) { gave_up = last == 2; break; }
  }
  if (gave_up) { if (tid == 0) status[0] = -3; return; }
  if (col0 + col < d)
    for (int r = slot; r < d; r += JR_SLOTS) Vt[int64_t(r) * ldv + col0 + col] = Vs[r * (JR_COLS + 1) + col];
}

template <int NB_>
__global__ __launch_bounds__(1024) void k_syev_chase(int d, const double* __restrict__ A, int64_t lda, double* __restrict__ w,
                                                     jac_cs* __restrict__ log, double tol, int max_sweeps, int* __restrict__ status,
                                                     unsigned* __restrict__ sync, double* __restrict__ Vt, int64_t ldv) {
  extern __shared__ __attribute__((aligned(16))) char jac_smem[];
  if (blockIdx.x == 0) {
    syev_packed_body<NB_>(jac_smem, d, A, lda, w, log, tol, max_sweeps, status, sync);
    return;
  }
  if (threadIdx.x >= 256) return;                              // (retired waves do not take part in the barriers of the rest)
  replay_chase_body(jac_smem, d, log, sync, Vt, ldv, int(blockIdx.x) - 1, status);
}

static size_t syev_small_lds(int64_t d) {
  const int64_t pe = (d + 1) & ~int64_t(1), np = pe / 2, sd = pe | 1;
  return size_t(2 * pe * sd + 18 + 4 * np) * 8;          // H, V', 16 maxima, 2 counters (+ pad), 2 x np (c, s)
}

static int syev_mode() { return env::once(env::SYEV_TWOSIDED); }

int syev_small_max(ccz_ctx*) { return syev_mode() == 2 ? 160 : (syev_mode() == 1 ? 96 : 0); }

int syev_small(ccz_ctx* c, const double* A, int64_t d, int64_t lda, double* w_dev, double* Vrows, int64_t ldv, int max_sweeps, double tol) {
  const int dmax = syev_small_max(c);
  if (d < 1 || d > dmax) fail(CCZ_EINVAL, "syev_small: 1 <= d <= %d required, got %lld", dmax, (long long)d);
  Impl* im = impl(c);
  int sw = 0;
  if (syev_mode() == 2) {
    const int64_t pe = (d + 1) & ~int64_t(1), m1 = pe - 1, np = pe / 2;
    const int64_t nH = pe * (pe + 1) / 2, nblk = np * (np + 1) / 2;
    const size_t lds_need = size_t(((nH + 1) & ~int64_t(1)) + 18 + 4 * np) * 8;
    DBuf logb(c, (int64_t(max_sweeps) * m1 + 1) * np * 2);
    jac_cs* log = reinterpret_cast<jac_cs*>(logb.get());
    auto launch = [&](auto kern) {
      CCZ_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, int(lds_need)));
      hipLaunchKernelGGL(kern, dim3(1), dim3(1024), lds_need, stream(c), int(d), A, lda, w_dev, log, tol,
                         max_sweeps, im->d_flag.get() + 2);
    };
    if (env::once(env::SYEV_CHASE) && Vrows) {
      // one launch: the solve and, next to it, the replay chasing its log (k_syev_chase)
      unsigned* sync = reinterpret_cast<unsigned*>(im->d_flag.get() + 32);      // (words 8 .. 15 are the pivot flags of the factorizations)
      CCZ_HIP(hipMemsetAsync(sync, 0, 2 * sizeof(unsigned), stream(c)));
      const size_t lds_chase = std::max(lds_need, size_t(160 * (JR_COLS + 1) * 8 + JR_CHUNK * 80 * 16 + 16));
      const dim3 grid(1u + unsigned((d + JR_COLS - 1) / JR_COLS));
      auto launch2 = [&](auto kern) {
        CCZ_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, int(lds_chase)));
        hipLaunchKernelGGL(kern, grid, dim3(1024), lds_chase, stream(c), int(d), A, lda, w_dev, log, tol, max_sweeps,
                           im->d_flag.get() + 2, sync, Vrows, ldv);
      };
      if (nblk <= 1024) launch2(&k_syev_chase<1>);
      else if (nblk <= 2048) launch2(&k_syev_chase<2>);
      else launch2(&k_syev_chase<4>);
      CCZ_LAUNCH_CHECK();
      int st[2] = {0, 0};
      d2h(c, st, im->d_flag.get() + 2, sizeof(st));
      sw = st[0];
      if (sw == -3) fail(CCZ_EHIP, "syev: the replaying workgroups lost the solving one");
      if (sw == -2) fail(CCZ_EINVAL, "syev: matrix has non-finite entries");
      if (sw < 0) fail(CCZ_ENOCONV, "Jacobi did not converge in %d sweeps (d=%lld)", max_sweeps, (long long)d);
      return sw;
    }
    if (nblk <= 1024) launch(&k_syev_packed1);
    else if (nblk <= 2048) launch(&k_syev_packed2);
    else launch(&k_syev_packed4);
    CCZ_LAUNCH_CHECK();
    int st[2] = {0, 0};
    d2h(c, st, im->d_flag.get() + 2, sizeof(st));
    sw = st[0];
    if (sw >= 1 && Vrows) {
      // the last sweep of a converged run rotated nothing: the log's first (sweeps - 1) * m1 rounds are all of V
      const int rounds = int((sw - 1) * m1);
      hipLaunchKernelGGL(k_jacobi_replay, dim3((unsigned)((d + JR_COLS - 1) / JR_COLS)), dim3(256), 0, stream(c), int(d), log, rounds,
                         Vrows, ldv);
      CCZ_LAUNCH_CHECK();     // (the log goes back to the handle's pool: reuse is ordered behind this launch on the same stream)
    }
  } else {
    const size_t lds_need = syev_small_lds(d);
    if (d <= 80) {
      CCZ_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(&k_syev_small), hipFuncAttributeMaxDynamicSharedMemorySize, int(lds_need)));
      hipLaunchKernelGGL(k_syev_small, dim3(1), dim3(1024), lds_need, stream(c), int(d), A, lda, w_dev, Vrows, ldv,
                         tol, max_sweeps, im->d_flag.get() + 1);
    } else {
      CCZ_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(&k_syev_small_wide), hipFuncAttributeMaxDynamicSharedMemorySize, int(lds_need)));
      hipLaunchKernelGGL(k_syev_small_wide, dim3(1), dim3(1024), lds_need, stream(c), int(d), A, lda, w_dev, Vrows, ldv,
                         tol, max_sweeps, im->d_flag.get() + 1);
    }
    CCZ_LAUNCH_CHECK();
    d2h(c, &sw, im->d_flag.get() + 1, sizeof(int));
  }
  if (sw == -2) fail(CCZ_EINVAL, "syev: matrix has non-finite entries");
  if (sw < 0) fail(CCZ_ENOCONV, "Jacobi did not converge in %d sweeps (d=%lld)", max_sweeps, (long long)d);
  return sw;
}

}  // namespace ccz
