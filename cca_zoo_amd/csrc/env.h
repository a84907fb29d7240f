// The runtime switches of libccz: ONE table, and the only getenv calls of the library.
//
// Every switch is an environment variable CCZ_<id>.  A row of the table is
//
//   X(id, kind, default, when, "values -- consumer: class; remarks")
//
//   kind   INT / I64 (atoi / atoll: text that is not a number reads as 0), REAL (atof), FLAG (set at all, whatever the value),
//          STR (the raw text, null when unset; the consumer parses it)
//   when   ONCE    on first use, then kept for the life of the process: a test must set it before a CHILD process starts
//          LIVE    on every call: setenv in the calling process acts on the next call (monkeypatch.setenv works)
//          LOAD    when libccz.so is loaded
//          HANDLE  in ccz_create, for that handle
//   class  knob (a deployment may set it), A/B (selects a measured alternative; the default won), test (lets a test reach
//          a path at a small size), trace (prints to stderr; never changes results)
//
// A site reads a switch through its row -- env::once(env::GRAM_MAP), env::live(env::SPLIT_ROWS) -- and the accessor has to match
// the row's `when` (checked at compile time; LOAD and HANDLE rows are read with live() at that one moment).  What is not
// parsing (a clamp, a unit, a text -> enum map) stays at the site.  Plain C++17: solve.cpp and the host test double use it.
#pragma once

#include <cstdlib>

namespace ccz {
namespace env {

enum When { ONCE, LIVE, LOAD, HANDLE };
using INT = int;
using I64 = long long;
using REAL = double;
using FLAG = bool;
using STR = const char*;

#define CCZ_ENV_TABLE(X)                                                                                                                      \
  /* ---- K1: second moments (gram.hip, gram_split.hip) ---- */                                                                               \
  X(K1_ROUTE, STR, nullptr, ONCE, "fp32 | bf16x2 (anything else: ignored) -- gram.hip launch_moments: knob; replaces CCZ_K1_AUTO of the handle for ccz_moments launches ONLY: the loss forward / backward and the projection look at the handle's route alone") \
  X(GRAM_MAP, INT, 1, ONCE, "1 chunk-per-XCD tile order, else the supertile order of round 2 -- gram.hip build_tile_table + plan_rows: A/B") \
  X(GRAM_ROWS, I64, 0, ONCE, "> 0: longest row chunk of a K1 workgroup (0: 16384) -- gram.hip plan_rows: A/B")                                \
  X(GRAM_PILOT, INT, -1, ONCE, "0 never / 1 always shift fp32 views by the pilot mean, else the caller's mode -- gram.hip launch_moments: test") \
  X(GRAM_PILOT_RATIO, REAL, 2.0, ONCE, "largest |mean| / std of a column that still runs unshifted -- gram.hip launch_moments: knob")          \
  X(GRAM_IMPL, INT, 1, ONCE, "fp32 K1: 0 register-staged shared tile, else wave-private FIFO -- gram.hip launch_moments: A/B")               \
  X(GRAM64_IMPL, INT, 1, ONCE, "fp64 K1: 0 staged, else FIFO -- gram.hip launch_moments: A/B")                                                \
  X(GRAM_FIFO_PILOT, INT, 1, ONCE, "0: pilot-shifted fp32 views take the staged kernel, not the FIFO one -- gram.hip launch_moments: A/B")    \
  X(GRAM_PARTIAL_MB, I64, 192, ONCE, "MiB of per-chunk partial tiles a launch may allocate instead of atomics (env::gram_partial_cap) -- gram.hip, gram_split.hip: knob") \
  X(LOSS_K1_FIFO, INT, 1, ONCE, "0: the loss's K1 partial sums come from the staged kernel -- gram.hip gram_partials_f32: A/B")               \
  X(H2D_CHUNK_MB, I64, 1024, LIVE, "MiB per row chunk of host-resident views (below 1: 1) -- gram.hip moments: knob; tests shrink it to get several chunks") \
  X(H2D_THREADS, INT, 0, LIVE, "host threads that pack a chunk (below 1: 1); UNSET: min(8, hardware threads) -- gram.hip moments: knob")      \
  X(H2D_PINNED_DIRECT, INT, 1, ONCE, "0: pinned host views are packed through the bounce buffers like pageable ones -- gram.hip moments: A/B") \
  X(SPLIT_MIN_FLOP, REAL, 1e11, LIVE, "flops from which the split-bf16 route pays -- gram_split.hip gram_split_worthwhile, gemm_split.hip gemm_split_pair_eligible (scales both of its thresholds): knob; tests lower it") \
  X(SPLIT_SCRATCH_GB, REAL, 48.0, LIVE, "GiB of scratch of a split-route launch (at most 0.4 of the device, at least 8 MiB) -- gram_split.hip split_scratch_budget: knob; tests shrink it to force several row super-chunks") \
  X(SPLIT_ROWS, I64, 16384, LIVE, "rows a split-route workgroup accumulates in fp32 -- gram_split.hip gram_split_f32: A/B; tests shorten it") \
  X(SPLIT_ORDER, INT, 1, LIVE, "0: row blocks fastest in the split pass's grid (the first form), else panels fastest -- gram_split.hip launch_split_pass: A/B") \
  X(SPLIT_WALK, INT, 0, LIVE, "1: every XCD walks the SAME row chunk also when ksplit % 8 == 0 -- gram_split.hip split_row_plan: A/B")       \
  X(LOSS_K1_SPLIT, INT, 1, LIVE, "0 never, 1 split-route partial sums from 32768 rows on, 2 and above from 4096 -- gram_split.hip gram_partials_split_f32: knob") \
  X(HALF_SCRATCH_MB, REAL, 256.0, LIVE, "MiB of float32 scratch a row chunk of CCZ_BF16 / CCZ_F16 views may take on the routes that widen them (fractions allowed; at least 4 KiB and 2 rows) -- half_io.hip half_chunk_rows: knob; tests shrink it to get several chunks") \
  /* ---- loss, projection, fp32 products (loss.hip, gemm_split.hip, project_split.hip, project_bf16.hip, gemm_big.hip) ---- */               \
  X(LOSS_FUSED, INT, 1, ONCE, "0: every shape takes the wide route (super-blocked factorization, 128-tile GEMMs) -- loss.hip narrow_ok: test") \
  X(LOSS_SPLITK, INT, 2, ONCE, "split-K factor of the narrow product stages (1 and below: none) -- loss.hip pair_core: A/B")                  \
  X(LOSS_FAST, INT, 1, ONCE, "0: the general route (moments + k_loss_prep) instead of K1's partial sums -- loss.hip forward: A/B")           \
  X(LOSS_BWD_SPLIT, INT, 1, LIVE, "0 never, 1 split-bf16 backward for the metric shape, 2 and above also DCCA batches from 4096 rows on -- gemm_split.hip gemm_split_pair_eligible: knob") \
  X(PROJECT_SPLIT, INT, 1, LIVE, "0: the projection keeps the fp32 kernel even on a CCZ_K1_BF16X2 handle -- project_split.hip project_split_eligible: A/B") \
  X(PROJECT_PLANES, INT, 2, LIVE, "3: three bf16 planes / five products, else two / three -- project_split.hip project_split: A/B")          \
  X(PROJECT_BF16, INT, 1, LIVE, "0: eligible CCZ_BF16 rows of ccz_transform_wide take the widening adapter, not the bf16 MFMA kernel -- project_bf16.hip project_bf16_eligible: A/B; tests reach the adapter with it") \
  X(TALL_IMPL, INT, 3, LIVE, "projection kernel: 3 whole-line loads with 128 rows per workgroup, 2 (and above 3) with 256 rows, below 2 a row per lane -- gemm_big.hip gemm_f32_big: A/B") \
  X(TALL_NJ1, INT, 1, LIVE, "0: two column tiles also for N <= 32 -- gemm_big.hip gemm_f32_big: A/B")                                        \
  X(GEMM_NN_IMPL, INT, 1, ONCE, "wide fp32 product: 0 staged tile, else LDS-DMA FIFO -- gemm_big.hip gemm_f32_big: A/B")                      \
  /* ---- fp64 GEMM (gemm64_big.hip, gemm64_skinny.hip) ---- */                                                                               \
  X(GEMM_BIG_MIN_TILES, I64, 32, ONCE, "128 x 128 tiles from which a product takes the big kernel -- gemm64_big.hip gemm_f64_big_eligible: A/B") \
  X(GEMM_BIG_MIN_K, I64, 64, ONCE, "smallest K of the big kernel -- gemm64_big.hip gemm_f64_big_eligible: A/B")                              \
  X(GEMM_HALF_TILE, I64, 1, ONCE, "0: no half-height tiles on grids smaller than the chip -- gemm64_big.hip gemm_f64_big: A/B")              \
  X(GEMM_SKINNY_OFF, STR, nullptr, ONCE, "text starting with 1: the skinny kernel is never eligible -- gemm64_skinny.hip gemm_f64_skinny_eligible: A/B") \
  /* ---- Cholesky and triangular solves (cholinv.hip, potrf.hip) ---- */                                                                     \
  X(CHOLINV_CHAIN, INT, 1, ONCE, "0: the launch-per-link form instead of the persistent chain kernel -- cholinv.hip chain_launch: A/B")      \
  X(CHAIN_WGS, INT, 128, ONCE, "workgroups of the chain launch (below 2: 2; Impl::chain_cap overrides it) -- cholinv.hip chain_launch: A/B")  \
  X(CHAIN_WGS_LA, INT, 64, ONCE, "the same on the look-ahead stream, next to the update GEMMs -- potrf.hip potrf_lower_batched_sb: A/B")     \
  X(CHAIN_SLEEP, INT, 1, ONCE, "sleep of the chain kernel's polling loops (below 1: 1) -- cholinv.hip chain_launch: A/B")                    \
  X(CHAIN_DEBUG, INT, 0, ONCE, "non-zero: shader-clock stamps of matrix 0's chain workgroup per launch (synchronises) -- cholinv.hip chain_launch: trace") \
  X(POTRF_SB, I64, 512, LOAD, "256 | 512 | 1024 (else: 512) columns per super-block; every user of the kept inverses sees one value -- potrf.hip SB: A/B")   \
  X(POTRF_LOOKAHEAD, INT, 1, ONCE, "0: the next super-block is factored on the handle's stream, not on a second one -- potrf.hip potrf_lookahead: A/B")   \
  X(POTRF_RIDER, INT, 1, ONCE, "0: the first whitening solve does not ride along the factorization -- potrf.hip potrf_lower_batched_aux_rider: A/B")   \
  X(BACKPROJ_SPLIT, INT, 4, ONCE, "split-K factor of the batched few-row solves -- potrf.hip trsm_right_lower_aux_multi: A/B")               \
  /* ---- eigensolvers (solve.cpp, syev_small.hip, evd_block.hip) ---- */                                                                     \
  X(EVD_REFRESH_MIN, INT, 1536, ONCE, "size from which the block Jacobi restarts from clean data near convergence -- evd_block.hip syev_block: knob") \
  X(BJ_GROUP_MIN_TILES, I64, 2048, ONCE, "row tiles from which a workgroup takes four 64-column chunks -- evd_block.hip bj_row_group: A/B")  \
  X(BJ_GRAM_SPLIT, INT, 0, ONCE, "column splits of the pair Gram products (below 1: 1); UNSET: sized to fill the chip -- evd_block.hip jacobi_rows_block: A/B") \
  X(BJ_DEBUG, FLAG, false, ONCE, "clock stamps of the pair kernel's three waves, printed in sweep 2 -- evd_block.hip syev_block: trace")     \
  X(SYEV_TWOSIDED, INT, 2, ONCE, "small EVD: 2 packed H + replayed V' (d <= 160), 1 fused LDS kernel (d <= 96), else no one-workgroup kernel: every size takes the block Jacobi of evd_block.hip -- syev_small.hip syev_mode: A/B") \
  X(SYEV_CHASE, INT, 1, ONCE, "0: the replay of V' is a launch of its own, not a chaser next to the solve -- syev_small.hip syev_small: A/B") \
  X(RR1_TOL, REAL, 1e-9, ONCE, "Jacobi threshold of the FIRST Rayleigh-Ritz (at or below 2.2e-16: full accuracy) -- solve.cpp topk_symmetric: A/B") \
  X(CHEB_MARGIN, REAL, 1e3, ONCE, "safety factor on the damping asked of the Chebyshev filter -- solve.cpp topk_symmetric: A/B")             \
  X(CHEB_MAXDEG, INT, 40, ONCE, "largest filter degree -- solve.cpp topk_symmetric: A/B")                                                    \
  X(CHEB_FIRSTCAP, INT, 28, ONCE, "largest degree of the first filter (below 2: 2) -- solve.cpp topk_symmetric: A/B")                        \
  /* ---- handle, host waits, communication (api.hip, runtime.hip, comm.hip) ---- */                                                          \
  X(GRAPHS, INT, 1, HANDLE, "0: launch chains are issued directly, never captured into hipGraphs -- api.hip ccz_create: A/B")               \
  X(SPIN_WAIT_MS, REAL, 50.0, ONCE, "milliseconds a short host wait polls before it blocks (0: always block) -- runtime.hip spin_budget_ms: knob") \
  X(D2H_MODE, INT, 0, LIVE, "small read-backs: 0 copy kernel with 8-byte lanes, 1 with 16-byte lanes, 2 hipMemcpyAsync + polled event, 3 + hipStreamSynchronize, 4 one blocking hipMemcpy -- runtime.hip d2h: A/B (tools/d2h_probe.py)") \
  X(RCCL_LIB, STR, nullptr, ONCE, "path of the one RCCL library to dlopen (read by the first communicator call) -- comm.hip rccl: knob; tests force the not-found path with it") \
  /* ---- traces ---- */                                                                                                                      \
  X(TRACE_PHASES, INT, 0, ONCE, "1 synchronise at phase boundaries and print wall times, 2 (rCCA solve only) events + shader clock without synchronising -- solve.cpp PhaseTimer (rcca, kcca, kgcca): trace") \
  X(TRACE_SOLVER, FLAG, false, ONCE, "Jacobi sweeps, cycles and filter degrees of the subspace iteration -- solve.cpp rayleigh_ritz, topk_symmetric: trace") \
  X(TRACE_POOL, FLAG, false, ONCE, "every hipMalloc behind a pool miss and every graph capture -- runtime.hip dev_alloc, graph_run: trace")  \
  X(TRACE_D2H, FLAG, false, LIVE, "device and host time of every small read-back -- runtime.hip d2h: trace")

#define CCZ_ENV_ROW(id, kind, dflt_, when_, doc)        \
  struct id##_t {                                       \
    using type = kind;                                  \
    static constexpr const char* name = "CCZ_" #id;     \
    static constexpr kind dflt = dflt_;                 \
    static constexpr When when = when_;                 \
  };                                                    \
  inline constexpr id##_t id{};
CCZ_ENV_TABLE(CCZ_ENV_ROW)
#undef CCZ_ENV_ROW

inline int parse(const char* e, int d) { return e ? atoi(e) : d; }
inline long long parse(const char* e, long long d) { return e ? atoll(e) : d; }
inline double parse(const char* e, double d) { return e ? atof(e) : d; }
inline bool parse(const char* e, bool) { return e != nullptr; }
inline const char* parse(const char* e, const char*) { return e; }

// the value now (LIVE rows; LOAD and HANDLE rows at their one moment)
template <class E> typename E::type live(E) {
  static_assert(E::when != ONCE, "this switch is read once per process: env::once");
  return parse(std::getenv(E::name), E::dflt);
}
// the value at the first call, for the life of the process (one cache per row, shared by all of its sites)
template <class E> typename E::type once(E) {
  static_assert(E::when == ONCE, "this switch is read at a moment of its own (see its row): env::live");
  static const typename E::type v = parse(std::getenv(E::name), E::dflt);
  return v;
}
// for the rows whose unset state is not a value ("UNSET:" in the row)
template <class E> bool is_set(E) { return std::getenv(E::name) != nullptr; }

inline long long gram_partial_cap() { return once(GRAM_PARTIAL_MB) << 20; }   // bytes

}  // namespace env
}  // namespace ccz
