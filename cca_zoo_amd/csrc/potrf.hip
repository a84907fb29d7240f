// HIP (gfx950 / CDNA4) implementation of the device-op interface in ops.h: potrf_lower*, trsm_right_lower*.
//
// Float64 dense linear algebra on d x d (d <= ~16k) blocks that lives AFTER the Gram reduction: it is latency /
// launch bound, not on the MFMA or HBM roofline (DESIGN.md "solver stage").  Cholesky / triangular solves are
// blocked around the GEMM (gemm64.hip and the kernels it dispatches to) and the step kernels of cholinv.hip.
#include <algorithm>
#include <vector>

#include "hip_common.h"

namespace ccz {

// ===========================================================================
// Cholesky (lower, blocked, right-looking) and right triangular solves
// ===========================================================================
constexpr int NB = 64;

// ---------------------------------------------------------------------------
// invT = L_bb^-T of every 64 x 64 diagonal block of a given lower factor L, each on ONE wavefront, no barriers.
// The block goes to LDS column-major (Ls[j][i] = L[i][j], stride 65); lane c then solves L x = e_c by forward
// substitution with its right-hand side in 64 registers consumed as a SHIFT REGISTER: at step t register v[0] is the
// current entry, the update writes its result one register down (v[k-1] = v[k] - L[t+k][t] x), so every register
// index is a compile-time constant while t is a run-time loop counter; the multipliers L[t+k][t] are wave-uniform
// LDS broadcasts.  Four loop bodies of decreasing width (63, 47, 31, 15 live entries) keep ~2/3 of the triangular
// saving without unrolling all 2016 (t, k) pairs -- straight-line code of that size does not fit the instruction
// cache.  Global loads / stores are whole 512-byte rows, transposed through LDS.  Blocks narrower than 64 are
// padded with the identity.
// ---------------------------------------------------------------------------
constexpr int WLD = NB + 1;   // LDS tile stride (doubles): column and row accesses both conflict-free

template <int KMAX>
__device__ __forceinline__ void inv_steps(double (&v)[NB], int t_begin, int t_end, int lane, const double* Ls, double* Xs) {
#pragma unroll 1
  for (int t = t_begin; t < t_end; ++t) {
    const double* lcol = Ls + t * WLD + t;         // L[t][t], L[t+1][t], ... (wave-uniform addresses)
    const double x = v[0] / lcol[0];
    Xs[lane * WLD + t] = x;                        // (L^-1)[t][lane] = (L^-T)[lane][t]
#pragma unroll
    for (int k = 1; k <= KMAX; ++k) {
      v[k - 1] = v[k] - lcol[k] * x;               // rows past 63: junk into registers that are never read
      if ((k & 7) == 0) __builtin_amdgcn_sched_barrier(0);
    }
    __builtin_amdgcn_sched_barrier(0);
  }
}

// Ljj: the diagonal block of L (row stride ldl), nb valid rows/columns.  invT: 64 x 64 row-major L_jj^-T.
__device__ __forceinline__ void diag_block_inv(const double* __restrict__ Ljj, int64_t ldl, int nb, double* __restrict__ invT, double* lds) {
  const int lane = threadIdx.x;
  double* Ls = lds;                 // Ls[t * WLD + i] = L[i][t]
  double* Xs = lds + NB * WLD;      // Xs[c * WLD + t] = (L^-T)[c][t]
  for (int r = 0; r < NB; ++r) {
    double v = (r == lane) ? 1.0 : 0.0;
    if (r < nb && lane < nb) v = lane <= r ? Ljj[int64_t(r) * ldl + lane] : 0.0;
    Ls[lane * WLD + r] = v;
  }
  double v[NB];
#pragma unroll
  for (int k = 0; k < NB; ++k) v[k] = (k == lane) ? 1.0 : 0.0;
  inv_steps<63>(v, 0, 16, lane, Ls, Xs);
  inv_steps<47>(v, 16, 32, lane, Ls, Xs);
  inv_steps<31>(v, 32, 48, lane, Ls, Xs);
  inv_steps<15>(v, 48, 64, lane, Ls, Xs);
  for (int r = 0; r < NB; ++r) invT[r * NB + lane] = Xs[r * WLD + lane];
}

constexpr size_t WAVE_BLOCK_LDS = (size_t(2) * NB * WLD + 2 * NB) * sizeof(double);   // two tiles + slack for the over-reads

__global__ __launch_bounds__(64) void k_diag_block_inv(const double* __restrict__ L, int64_t ldl, int64_t d, double* __restrict__ invT) {
  extern __shared__ __attribute__((aligned(16))) char wave_smem[];
  const int64_t j0 = int64_t(blockIdx.x) * NB;
  const int nb = int(min(int64_t(NB), d - j0));
  diag_block_inv(L + j0 * ldl + j0, ldl, nb, invT + int64_t(blockIdx.x) * NB * NB, reinterpret_cast<double*>(wave_smem));
}

// the wave kernel uses 65 KiB of dynamic LDS: opt in once per device (never inside a graph capture)
void wave_kernels_init() {
  static thread_local int done_for_device = -1;
  int dev = -1;
  CCZ_HIP(hipGetDevice(&dev));
  if (done_for_device == dev) return;
  CCZ_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(&k_diag_block_inv), hipFuncAttributeMaxDynamicSharedMemorySize, int(WAVE_BLOCK_LDS)));
  done_for_device = dev;
}

// invT[b] = L_bb^-T for every diagonal block b of L (one wave each, all blocks in one launch)
static void diag_inverses(ccz_ctx* c, const double* L, int64_t ldl, int64_t d, double* invT) {
  const unsigned nblk = (unsigned)((d + NB - 1) / NB);
  hipLaunchKernelGGL(k_diag_block_inv, dim3(nblk), dim3(64), WAVE_BLOCK_LDS, stream(c), L, ldl, d, invT);
  CCZ_LAUNCH_CHECK();
}

int potrf_lower(ccz_ctx* c, double* A, int64_t d, int64_t lda) {
  int info = 0;
  double* Ap[1] = {A};
  potrf_lower_batched(c, 1, Ap, &d, &lda, &info);
  return info;
}

static inline uint64_t key_ptr(uint64_t h, const void* p) { return graph_key_mix(h, reinterpret_cast<uint64_t>(p)); }

// d < 1024: one 64-column block at a time against the explicit L_jj^-T of the diagonal blocks
static void trsm_right_lower_iter(ccz_ctx* c, bool trans, int64_t r, int64_t d, const double* L, int64_t ldl, double* X,
                      int64_t ldx) {
  if (r <= 0 || d <= 0) return;
  const int64_t nblk = (d + NB - 1) / NB;
  DBuf invT(c, nblk * NB * NB), tmp(c, r * NB);
  uint64_t key = graph_key_mix(0x5452534dull, uint64_t(trans));
  key = graph_key_mix(graph_key_mix(key, uint64_t(r)), uint64_t(d));
  key = graph_key_mix(graph_key_mix(key_ptr(key_ptr(key, L), X), uint64_t(ldl)), uint64_t(ldx));
  key = key_ptr(key_ptr(key, invT.get()), tmp.get());
  // A graph is keyed on every pointer baked into it; capture + instantiation cost ~10 ms.  The few-block solves of the
  // subspace iteration (d = 80: two blocks, five launches) meet new pointer combinations whenever the pool hands out
  // other blocks -- the second fit of a new shape paid 20 ms for graphs that save nothing.  Replay only pays for long chains.
  auto body = [&] {
  diag_inverses(c, L, ldl, d, invT);
  if (trans) {
    // X L' = B, forward over column blocks:  X_j = (B_j - sum_{t<j} X_t L_jt') L_jj^-T
    for (int64_t bj = 0; bj < nblk; ++bj) {
      const int64_t j = bj * NB;
      const int nb = int(std::min<int64_t>(NB, d - j));
      gemm_ex(c, false, false, r, nb, nb, 1.0, X + j, ldx, invT.get() + bj * NB * NB, NB, 0.0, tmp, NB, X + j, ldx, false);
      const int64_t rem = d - j - nb;
      if (rem > 0)  // X[:, j+nb:] -= X_j  L[j+nb:, j]'
        gemm(c, false, true, r, rem, nb, -1.0, tmp, NB, L + (j + nb) * ldl + j, ldl, 1.0, X + j + nb, ldx);
    }
  } else {
    // X L = B, backward:  X_j = (B_j - sum_{t>j} X_t L_tj) L_jj^-1 ;  L_jj^-1 = (invT_j)'
    for (int64_t bj = nblk - 1; bj >= 0; --bj) {
      const int64_t j = bj * NB;
      const int nb = int(std::min<int64_t>(NB, d - j));
      gemm_ex(c, false, true, r, nb, nb, 1.0, X + j, ldx, invT.get() + bj * NB * NB, NB, 0.0, tmp, NB, X + j, ldx, false);
      if (j > 0)  // X[:, :j] -= X_j L[j:j+nb, :j]
        gemm(c, false, false, r, j, nb, -1.0, tmp, NB, L + j * ldl, ldl, 1.0, X, ldx);
    }
  }
  };
  if (nblk >= 8) graph_run_fn(c, key, body);
  else body();
}


// ---------------------------------------------------------------------------
// Round-2 paths (cholinv.hip):
//  * potrf: the step kernels with look-ahead -- ONE launch per 64-column block for all matrices of the batch (the
//    trailing tiles recompute their panel blocks, the owner of the next diagonal block factors it in the same
//    launch) instead of three launches and a 60 us single-wave factorization per block; above 4096 columns the
//    3x recompute of the tiles costs more than it saves and the factorization runs on 512-column super-blocks
//    (batched step kernels on the diagonal super-blocks, 128-tile GEMMs for panel and trailing update).
//  * trsm: 512-column super-blocks with explicit inverses of the diagonal super-blocks (one batched pass of the
//    inverse rows) -- 8 x (r x 512 x 512 product + rank-512 trailing update) at the big-GEMM rate instead of 64
//    rank-64 updates that were bound by HBM.
// ---------------------------------------------------------------------------
static const int64_t SB = [] {
  const int64_t v = env::live(env::POTRF_SB);
  return (v == 256 || v == 1024) ? v : int64_t(512);
}();

static void potrf_lower_batched_steps(ccz_ctx* c, int count, double* const* A, const int64_t* d, const int64_t* lda, int* info) {
  for (int b0 = 0; b0 < count; b0 += 8) {
    const int nbt = std::min(8, count - b0);
    std::vector<DBuf> Lb(nbt), Tb(nbt);
    std::vector<double*> Lp(nbt), Tp(nbt);
    std::vector<int64_t> ldl(nbt);
    for (int i = 0; i < nbt; ++i) {
      const int64_t di = d[b0 + i];
      Lb[i] = DBuf(c, di * di);
      Tb[i] = DBuf(c, (di + NB - 1) / NB * NB * NB);
      Lp[i] = Lb[i].get();
      Tp[i] = Tb[i].get();
      ldl[i] = di;
    }
    int* info_dev = impl(c)->d_flag.get() + 8;
    cholinv_batched(c, nbt, A + b0, lda + b0, d + b0, Lp.data(), ldl.data(), nullptr, nullptr, Tp.data(), info_dev);
    for (int i = 0; i < nbt; ++i) copy_lower(c, d[b0 + i], Lp[i], ldl[i], A[b0 + i], lda[b0 + i]);
    int got[8];
    d2h(c, got, info_dev, size_t(nbt) * sizeof(int));
    for (int i = 0; i < nbt; ++i) info[b0 + i] = got[i] == 0x7fffffff ? 0 : got[i];
  }
}

// d > 1024: right-looking over 512-column super-blocks, all matrices of the batch together -- the diagonal
// super-blocks of every matrix are factored (+ inverted) in ONE batched pass of the step kernels (the chain of nine
// dependent launches is shared), panel and trailing update are 128-tile GEMMs with K = 512.  (The step kernels
// alone on a 4096-column matrix are rank-64 updates of the whole trailing matrix -- HBM-bound, measured 8 ms for two
// matrices; the super-blocked form moves 8x less.)  Pivot failures are collected at the end: one host read.
//
// Look-ahead: super-block J + 1 can be factored as soon as ITS diagonal block has received update J, i.e. after the
// top 512 rows of panel J -- not after the whole trailing update.  The factorization is a latency chain on a handful
// of workgroups, the rest of the update is throughput work, so the chain moves to a second stream and the two overlap:
//   main:  copy L_JJ | panel top | diag (J+1,J+1) update | ev_a | panel rest | column J+1 | trailing rest | wait ev_b
//   aux :                                      wait ev_a | factor + invert (J+1,J+1) ......................| ev_b
// CCZ_POTRF_LOOKAHEAD=0 keeps everything on the handle's stream (same order of operations).
//
// keep[i] (optional, nsb * 512 * 512 doubles): receives the inverses of matrix i's diagonal super-blocks for later
// triangular solves with the factor (trsm_right_lower_aux).
static int potrf_lookahead() { return env::once(env::POTRF_LOOKAHEAD); }

struct StreamSwap {
  ccz_ctx* c;
  void* prev;
  StreamSwap(ccz_ctx* c_, hipStream_t s) : c(c_), prev(c_->stream) { c->stream = s; }
  ~StreamSwap() { c->stream = prev; }
};

static void potrf_lower_batched_sb(ccz_ctx* c, int count, double* const* A, const int64_t* d, const int64_t* lda, int* info,
                                   double* const* keep, const TrsmRider* rider = nullptr, int rider_idx = -1) {
  if (count > 8) fail(CCZ_EUNSUP, "potrf_lower_batched_sb: at most 8 matrices per call");
  // the rider's r x 512 product buffer (X_J inv(L_JJ)') -- see the end of the J loop
  DBuf rtmp;
  if (rider) rtmp = DBuf(c, rider->r * SB);
  Impl* im = impl(c);
  int64_t dmax = 0;
  for (int i = 0; i < count; ++i) dmax = std::max(dmax, d[i]);
  const int64_t nsb = (dmax + SB - 1) / SB;
  std::vector<DBuf> Ld(count), Xv(count), Tv(count);
  for (int i = 0; i < count; ++i) {
    Ld[i] = DBuf(c, SB * SB);
    Tv[i] = DBuf(c, (SB / NB) * NB * NB);
    // the panel products read whole blocks; the inverse rows overwrite only the lower blocks
    if (keep && keep[i]) {
      zero(c, keep[i], size_t((d[i] + SB - 1) / SB) * SB * SB * 8);
    } else {
      Xv[i] = DBuf(c, 2 * SB * SB);       // two halves: factor(J + 1) writes one while update J still reads the other
      zero(c, Xv[i], size_t(2) * SB * SB * 8);
    }
  }
  // info of super-step J of matrix i: slot J * 8 + (position among the matrices alive at J); all start at "no failure"
  const int nslots = int(nsb) * 8;
  PoolBuf<int> info_dev(c, nslots);
  // Unwinding (an allocation or launch failure between the look-ahead launch and the main stream's wait): the pooled
  // buffers above go back to the pool as they unwind, and the pool recycles them in the order of the MAIN stream --
  // so the look-ahead stream must be drained first: this is declared after them, hence unwinds before them.
  struct Unwind {
    Impl* im; bool armed = true;
    ~Unwind() { if (armed && im->aux) (void)hipStreamSynchronize(im->aux->st.get()); }
  } unwind{im};

  hipStream_t s_main = stream(c), s_aux = s_main;
  bool la = potrf_lookahead() != 0 && nsb > 1;
  if (la) {
    if (!im->aux && !make_side_stream(im->aux)) la = false;
    if (la) s_aux = im->aux->st.get();
  }
  const hipEvent_t aux_ev[2] = {la ? im->aux->ev[0].get() : nullptr, la ? im->aux->ev[1].get() : nullptr};

  // diagonal super-block J of every matrix still alive: factor, invert (on the CURRENT c->stream)
  auto factor = [&](int64_t J) {
    const int64_t j0 = J * SB;
    double* Ap[8]; double* Lp[8]; double* Xp[8]; double* Tp[8];
    int64_t la_[8], dd[8], ll[8];
    int cnt = 0;
    bool need_x = false;
    for (int i = 0; i < count; ++i) {
      if (j0 >= d[i]) continue;
      Ap[cnt] = A[i] + j0 * lda[i] + j0;
      la_[cnt] = lda[i];
      dd[cnt] = std::min(SB, d[i] - j0);
      Lp[cnt] = Ld[i].get();
      Xp[cnt] = (keep && keep[i]) ? keep[i] + J * SB * SB : Xv[i].get() + (J & 1) * SB * SB;
      Tp[cnt] = Tv[i].get();
      ll[cnt] = SB;
      need_x = need_x || (keep && keep[i]) || d[i] - j0 - dd[cnt] > 0;
      ++cnt;
    }
    if (cnt > 0) cholinv_batched(c, cnt, Ap, la_, dd, Lp, ll, need_x ? Xp : nullptr, ll, Tp, info_dev + J * 8);
  };

  factor(0);
  for (int64_t J = 0; J < nsb; ++J) {
    const int64_t j0 = J * SB;
    std::vector<DBuf> tmp(count);
    // ---- the part super-block J + 1 waits for: top block of panel J and the update of diagonal block J + 1.
    // Two 512^3 products per matrix -- far too small for a launch each (40 us on 64 workgroups): one batched,
    // split-K launch per stage for all matrices (512 workgroups, ~12 us)
    {
      MultiGemmArgs top[8], dg[8];
      int nt = 0;
      for (int i = 0; i < count; ++i) {
        if (j0 >= d[i]) continue;
        const int64_t w = std::min(SB, d[i] - j0), rem = d[i] - j0 - w;
        copy_lower(c, w, Ld[i], SB, A[i] + j0 * lda[i] + j0, lda[i]);
        if (rem <= 0) continue;
        const int64_t w1 = std::min(SB, rem);
        const double* Xj = (keep && keep[i]) ? keep[i] + J * SB * SB : Xv[i].get() + (J & 1) * SB * SB;
        tmp[i] = DBuf(c, rem * w);
        zero(c, tmp[i], size_t(w1) * w * 8);
        MultiGemmArgs& a = top[nt];                                                     // top of L21 = A21 L11^-T
        a = MultiGemmArgs{};
        a.A = A[i] + (j0 + w) * lda[i] + j0; a.lda = lda[i]; a.tA = false;
        a.B = Xj; a.ldb = SB; a.tB = true;
        a.C = tmp[i]; a.ldc = w; a.Ct = nullptr; a.ldct = 0;
        a.M = w1; a.N = w; a.K = w; a.alpha = 1.0; a.beta = 1.0; a.lower_only = false; a.ksplit = 4;
        MultiGemmArgs& b = dg[nt];                                                      // A(J+1,J+1) -= top top'
        b = MultiGemmArgs{};
        b.A = tmp[i]; b.lda = w; b.tA = false;
        b.B = tmp[i]; b.ldb = w; b.tB = true;
        b.C = A[i] + (j0 + w) * lda[i] + (j0 + w); b.ldc = lda[i]; b.Ct = nullptr; b.ldct = 0;
        b.M = w1; b.N = w1; b.K = w; b.alpha = -1.0; b.beta = 1.0; b.lower_only = true; b.ksplit = 4;
        ++nt;
      }
      if (nt > 0) {
        gemm_f64_multi(c, nt, top);
        gemm_f64_multi(c, nt, dg);
      }
    }
    if (J + 1 < nsb) {
      if (la) {
        CCZ_HIP(hipEventRecord(aux_ev[0], s_main));
        CCZ_HIP(hipStreamWaitEvent(s_aux, aux_ev[0], 0));
        {
          StreamSwap sw(c, s_aux);
          // the chain kernel's helper workgroups spin while they wait: next to the update GEMMs of the main stream they get a
          // bounded share of the chip
          const int cap0 = im->chain_cap;
          im->chain_cap = env::once(env::CHAIN_WGS_LA);
          try { factor(J + 1); } catch (...) { im->chain_cap = cap0; throw; }
          im->chain_cap = cap0;
        }
        CCZ_HIP(hipEventRecord(aux_ev[1], s_aux));
      } else {
        factor(J + 1);
      }
    }
    // ---- the rest of update J (overlaps the factorization of super-block J + 1) ----
    for (int i = 0; i < count; ++i) {
      if (j0 >= d[i]) continue;
      const int64_t w = std::min(SB, d[i] - j0), rem = d[i] - j0 - w;
      if (rem <= 0) continue;
      const int64_t w1 = std::min(SB, rem), rem2 = rem - w1;
      const int64_t j1 = j0 + w;
      copy2d(c, w1, w, tmp[i], w, A[i] + j1 * lda[i] + j0, lda[i]);                                  // top of L21 -> the factor
      if (rem2 <= 0) continue;
      double* A31 = A[i] + (j1 + w1) * lda[i] + j0;
      double* t2 = tmp[i].get() + w1 * w;
      const double* Xj = (keep && keep[i]) ? keep[i] + J * SB * SB : Xv[i].get() + (J & 1) * SB * SB;
      gemm(c, false, true, rem2, w, w, 1.0, A31, lda[i], Xj, SB, 0.0, t2, w);                       // rest of L21
      copy2d(c, rem2, w, t2, w, A31, lda[i]);
      gemm(c, false, true, rem2, w1, w, -1.0, t2, w, tmp[i], w, 1.0, A[i] + (j1 + w1) * lda[i] + j1, lda[i]);   // column J + 1
      gemm_ex(c, false, true, rem2, rem2, w, -1.0, t2, w, t2, w, 1.0, A[i] + (j1 + w1) * lda[i] + (j1 + w1), lda[i], nullptr, 0, true);
    }
    // ---- the rider: column block J of its factor is final now (diagonal block, panel top, panel rest), so step J of
    // X <- X L^-T can go: X_J <- X_J inv(L_JJ)', X[:, below] -= X_J L[below, J]'  (trsm_right_lower_sb, trans branch).
    // It queues behind update J on the main stream -- throughput work under the factorization chain of block J + 1.
    if (rider && j0 < d[rider_idx]) {
      const int i = rider_idx;
      if (J == 0 && rider->prepare) rider->prepare();
      const int64_t w = std::min(SB, d[i] - j0), rem = d[i] - j0 - w;
      const double* Xinv = keep[i] + J * SB * SB;
      double* X = rider->X;
      gemm(c, false, true, rider->r, w, w, 1.0, X + j0, rider->ldx, Xinv, SB, 0.0, rtmp, SB);
      copy2d(c, rider->r, w, rtmp, SB, X + j0, rider->ldx);
      if (rem > 0)
        gemm(c, false, true, rider->r, rem, w, -1.0, rtmp, SB, A[i] + (j0 + w) * lda[i] + j0, lda[i], 1.0, X + j0 + w, rider->ldx);
    }
    if (la && J + 1 < nsb) CCZ_HIP(hipStreamWaitEvent(s_main, aux_ev[1], 0));
  }
  std::vector<int> got(nslots, 0x7fffffff);
  // slots of (J, t) with t >= cnt of that super-step were never written: only read what cholinv_batched initialised
  d2h(c, got.data(), info_dev, size_t(nslots) * sizeof(int));
  unwind.armed = false;
  info_dev.reset();
  for (int i = 0; i < count; ++i) info[i] = 0;
  for (int64_t J = 0; J < nsb; ++J) {
    int cnt = 0;
    for (int i = 0; i < count; ++i) {
      if (J * SB >= d[i]) continue;
      const int v = got[J * 8 + cnt];
      if (v != 0x7fffffff && info[i] == 0) info[i] = int(J * SB) + v;
      ++cnt;
    }
  }
}

// Dispatch of every factorization: matrices up to 1024 columns go through the step kernels directly; wider ones super-blocked;
// both batched by 8.  Returns whether the rider rode along.
static bool potrf_dispatch(ccz_ctx* c, int count, double* const* A, const int64_t* d, const int64_t* lda, int* info,
                           double* const* aux, const TrsmRider* rider) {
  std::vector<double*> As, Ab, Kb;
  std::vector<int64_t> ds, lds_, db, ldb_;
  std::vector<int> idx, idb;
  for (int i = 0; i < count; ++i) {
    if (d[i] <= 1024) { As.push_back(A[i]); ds.push_back(d[i]); lds_.push_back(lda[i]); idx.push_back(i); }
    else { Ab.push_back(A[i]); db.push_back(d[i]); ldb_.push_back(lda[i]); idb.push_back(i); Kb.push_back(aux ? aux[i] : nullptr); }
  }
  if (!As.empty()) {
    std::vector<int> inf(As.size(), 0);
    potrf_lower_batched_steps(c, int(As.size()), As.data(), ds.data(), lds_.data(), inf.data());
    for (size_t t = 0; t < idx.size(); ++t) info[idx[t]] = inf[t];
  }
  bool rode = false;
  for (size_t b0 = 0; b0 < Ab.size(); b0 += 8) {
    const int nbt = int(std::min<size_t>(8, Ab.size() - b0));
    int inf[8];
    // the rider needs the kept inverses of its factor's diagonal super-blocks
    int ridx = -1;
    if (rider && rider->X && rider->r > 0)
      for (int t = 0; t < nbt; ++t)
        if (idb[b0 + t] == rider->matrix && Kb[b0 + t]) ridx = t;
    potrf_lower_batched_sb(c, nbt, Ab.data() + b0, db.data() + b0, ldb_.data() + b0, inf, Kb.data() + b0, ridx >= 0 ? rider : nullptr, ridx);
    rode = rode || ridx >= 0;
    for (int t = 0; t < nbt; ++t) info[idb[b0 + t]] = inf[t];
  }
  return rode;
}

static void trsm_right_lower_sb(ccz_ctx* c, bool trans, int64_t r, int64_t d, const double* L, int64_t ldl, double* X, int64_t ldx,
                                const double* aux = nullptr) {
  const int64_t nblk = (d + NB - 1) / NB, nsb = (d + SB - 1) / SB;
  DBuf tmp(c, r * SB), Xown;
  const double* Xinv = aux;                                    // inverses of the diagonal super-blocks, kept by potrf
  if (!Xinv) {
    DBuf invT(c, nblk * NB * NB);
    Xown = DBuf(c, nsb * SB * SB);
    diag_inverses(c, L, ldl, d, invT);                         // L_jj^-T of every 64-column block, one launch
    zero(c, Xown, size_t(nsb) * SB * SB * 8);                  // the products read whole super-blocks
    for (int64_t J0 = 0; J0 < nsb; J0 += 8) {
      const int cnt = int(std::min<int64_t>(8, nsb - J0));
      const double* Lp[8];
      const double* Tp[8];
      double* Xp[8];
      int64_t dd[8], l1[8], l2[8];
      for (int t = 0; t < cnt; ++t) {
        const int64_t j0 = (J0 + t) * SB;
        Lp[t] = L + j0 * ldl + j0;
        Tp[t] = invT.get() + (j0 / NB) * NB * NB;
        Xp[t] = Xown.get() + (J0 + t) * SB * SB;
        dd[t] = std::min(SB, d - j0);
        l1[t] = ldl;
        l2[t] = SB;
      }
      trinv_batched(c, cnt, Lp, l1, dd, Xp, l2, Tp);
    }
    Xinv = Xown.get();
  }
  if (trans) {
    // X L' = B, forward over the super-blocks:  X_J = (B_J - sum_{t<J} X_t L_Jt') L_JJ^-T
    for (int64_t J = 0; J < nsb; ++J) {
      const int64_t j0 = J * SB, w = std::min(SB, d - j0), rem = d - j0 - w;
      gemm(c, false, true, r, w, w, 1.0, X + j0, ldx, Xinv + J * SB * SB, SB, 0.0, tmp, SB);
      copy2d(c, r, w, tmp, SB, X + j0, ldx);
      if (rem > 0) gemm(c, false, true, r, rem, w, -1.0, tmp, SB, L + (j0 + w) * ldl + j0, ldl, 1.0, X + j0 + w, ldx);
    }
  } else {
    // X L = B, backward:  X_J = (B_J - sum_{t>J} X_t L_tJ) L_JJ^-1
    for (int64_t J = nsb - 1; J >= 0; --J) {
      const int64_t j0 = J * SB, w = std::min(SB, d - j0);
      gemm(c, false, false, r, w, w, 1.0, X + j0, ldx, Xinv + J * SB * SB, SB, 0.0, tmp, SB);
      copy2d(c, r, w, tmp, SB, X + j0, ldx);
      if (j0 > 0) gemm(c, false, false, r, j0, w, -1.0, tmp, SB, L + j0 * ldl, ldl, 1.0, X, ldx);
    }
  }
}

void potrf_lower_batched(ccz_ctx* c, int count, double* const* A, const int64_t* d, const int64_t* lda, int* info) {
  potrf_dispatch(c, count, A, d, lda, info, nullptr, nullptr);
}

// Factor and inverse of ONE small SPD matrix (ops.h): the chain kernel produces L^-1 next to L (cholinv_batched with X), so the
// Cholesky-QR passes of the subspace iteration need no triangular solve -- X <- X L^-T is one product with the explicit inverse.
int potrf_lower_inv(ccz_ctx* c, double* A, int64_t d, int64_t lda, double* Linv, int64_t ldi) {
  if (d < 1) fail(CCZ_EINVAL, "potrf_lower_inv: d >= 1 required");
  if (d > 4096) {
    // (no chain kernel: factor, then L^-1 = I L^-1 by the triangular solve)
    const int info = potrf_lower(c, A, d, lda);
    if (info != 0) return info;
    fill2d(c, d, d, Linv, ldi, 0.0);
    add_diag(c, d, Linv, ldi, 1.0);
    trsm_right_lower(c, false, d, d, A, lda, Linv, ldi);
    return 0;
  }
  DBuf Lb(c, d * d), Tb(c, (d + NB - 1) / NB * NB * NB);
  double* Ap[1] = {A};
  double* Lp[1] = {Lb.get()};
  double* Xp[1] = {Linv};
  double* Tp[1] = {Tb.get()};
  const int64_t dd[1] = {d}, la[1] = {lda}, ll[1] = {d}, lx[1] = {ldi};
  fill2d(c, d, d, Linv, ldi, 0.0);                     // (the chain writes the lower triangle only)
  int* info_dev = impl(c)->d_flag.get() + 8;
  cholinv_batched(c, 1, Ap, la, dd, Lp, ll, Xp, lx, Tp, info_dev);
  int got = 0;
  d2h(c, &got, info_dev, sizeof(int));
  return got == 0x7fffffff ? 0 : got;
}

int64_t trsm_aux_size(ccz_ctx*, int64_t d) {
  if (d <= 1024) return 0;
  return (d + SB - 1) / SB * SB * SB;
}

void potrf_lower_batched_aux(ccz_ctx* c, int count, double* const* A, const int64_t* d, const int64_t* lda, int* info,
                             double* const* aux) {
  potrf_dispatch(c, count, A, d, lda, info, aux, nullptr);
}

bool potrf_lower_batched_aux_rider(ccz_ctx* c, int count, double* const* A, const int64_t* d, const int64_t* lda, int* info,
                                   double* const* aux, const TrsmRider* rider) {
  if (!aux || !env::once(env::POTRF_RIDER)) rider = nullptr;
  return potrf_dispatch(c, count, A, d, lda, info, aux, rider);
}

void trsm_right_lower_aux(ccz_ctx* c, bool trans, int64_t r, int64_t d, const double* L, int64_t ldl, double* X,
                          int64_t ldx, const double* aux) {
  if (r <= 0 || d <= 0) return;
  if (aux && d > 1024) { trsm_right_lower_sb(c, trans, r, d, L, ldl, X, ldx, aux); return; }
  trsm_right_lower(c, trans, r, d, L, ldl, X, ldx);
}

void trsm_right_lower(ccz_ctx* c, bool trans, int64_t r, int64_t d, const double* L, int64_t ldl, double* X,
                      int64_t ldx) {
  if (r <= 0 || d <= 0) return;
  if (d >= 1024) trsm_right_lower_sb(c, trans, r, d, L, ldl, X, ldx);
  else trsm_right_lower_iter(c, trans, r, d, L, ldl, X, ldx);
}

// Few-row solves of several problems together (back-projection of the k wanted directions through every view's
// factor).  One problem alone is 2 dependent launches per super-block, each a 64-row product that cannot fill the chip
// (31 us apiece, 16 per 4096-column factor); here every step is two batched split-K launches for ALL problems:
//   stage 1:  Y_b[:, J] += X_b[:, J] inv(L_b,JJ)^(T)           (Y zeroed once; result accumulates out of place)
//   stage 2:  X_b[:, rest] -= Y_b[:, J] L_b[., .]^(T)            (the not yet solved columns)
void trsm_right_lower_aux_multi(ccz_ctx* c, int count, bool trans, const int64_t* r, const int64_t* d, const double* const* L,
                                const int64_t* ldl, double* const* X, const int64_t* ldx, const double* const* aux) {
  bool batched = count >= 1 && count <= 8;
  for (int b = 0; b < count && batched; ++b) batched = aux && aux[b] && d[b] > 1024 && r[b] >= 1 && r[b] <= 256;
  if (!batched) {
    for (int b = 0; b < count; ++b) trsm_right_lower_aux(c, trans, r[b], d[b], L[b], ldl[b], X[b], ldx[b], aux ? aux[b] : nullptr);
    return;
  }
  const int bp_split = env::once(env::BACKPROJ_SPLIT);
  int64_t total = 0, offs[8], nsb[8], max_nsb = 0;
  for (int b = 0; b < count; ++b) {
    offs[b] = total;
    total += r[b] * d[b];
    nsb[b] = (d[b] + SB - 1) / SB;
    max_nsb = std::max(max_nsb, nsb[b]);
  }
  DBuf Y(c, total);
  zero(c, Y, size_t(total) * 8);
  for (int64_t st = 0; st < max_nsb; ++st) {
    MultiGemmArgs s1[8], s2[8];
    int n1 = 0, n2 = 0;
    for (int b = 0; b < count; ++b) {
      if (st >= nsb[b]) continue;
      const int64_t J = trans ? st : nsb[b] - 1 - st;
      const int64_t j0 = J * SB, w = std::min(SB, d[b] - j0);
      double* Yb = Y.get() + offs[b];
      MultiGemmArgs& a = s1[n1++];
      a = MultiGemmArgs{};
      a.A = X[b] + j0; a.lda = ldx[b]; a.tA = false;
      a.B = aux[b] + J * SB * SB; a.ldb = SB; a.tB = trans;
      a.C = Yb + j0; a.ldc = d[b]; a.Ct = nullptr; a.ldct = 0;
      a.M = r[b]; a.N = w; a.K = w; a.alpha = 1.0; a.beta = 1.0; a.lower_only = false; a.ksplit = bp_split;
      const int64_t rest = trans ? d[b] - j0 - w : j0;
      if (rest <= 0) continue;
      MultiGemmArgs& u = s2[n2++];
      u = MultiGemmArgs{};
      u.A = Yb + j0; u.lda = d[b]; u.tA = false;
      if (trans) { u.B = L[b] + (j0 + w) * ldl[b] + j0; u.tB = true; u.C = X[b] + j0 + w; }      // X[:, below] -= Y_J L[below, J]'
      else { u.B = L[b] + j0 * ldl[b]; u.tB = false; u.C = X[b]; }                                  // X[:, :j0]  -= Y_J L[J, :j0]
      u.ldb = ldl[b]; u.ldc = ldx[b]; u.Ct = nullptr; u.ldct = 0;
      u.M = r[b]; u.N = rest; u.K = w; u.alpha = -1.0; u.beta = 1.0; u.lower_only = false; u.ksplit = bp_split;
    }
    if (n1 > 0) gemm_f64_multi(c, n1, s1);
    if (n2 > 0) gemm_f64_multi(c, n2, s2);
  }
  for (int b = 0; b < count; ++b) copy2d(c, r[b], d[b], Y.get() + offs[b], d[b], X[b], ldx[b]);
}

}  // namespace ccz
