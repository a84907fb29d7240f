// ProbabilisticCCA: the No-U-Turn sampler, whole leapfrog steps on the device.
//
// The algorithm is written down in include/ccz.h (the ccz_nuts_* section) and restated in NumPy in tests/pcca_restatement.py,
// which is the specification.  The state is one flat vector of N = ptot K + ptot + n K doubles:
//   [ W of all views back to back (ptot x K, row-major) | s = log psi of all views (ptot) | Z (n x K) ]
// and the momentum, the gradient and every adaptation vector share that layout.  Device vectors live in numbered slots (NutsSlot
// below): the tree's two ends (q, p, g each), the chain's point and the subtree's proposal (q, g each), the momentum sums of the
// tree and of the subtree under construction, minv, the Welford mean and M2, and per tree level one checkpoint (p, momentum sum).
//
// One leapfrog from the tree's end `side`, for M views:
//   k_nuts_kick             p -= (eps / 2) g;  q += eps minv o p                                        one pass over N
//   per view i:
//     k_svi_fused_*         ONE read of X_i (svi_fused.h, shared with svi.hip): the partials of D' Z, D W_i, sum R^2 exp(-2 s)
//   k_nuts_fold             the partials folded in index order into g, the prior terms, p -= (eps / 2) g, the subtree's momentum
//                           sum, the checkpoint of an even leaf, and per-workgroup partials of U, of the kinetic energy and
//                           of the dot products of every U-turn test this leaf closes                   one pass over N
//   k_nuts_finish           one workgroup: the partials folded in a fixed order into the record {U, kinetic, H, dots, finite}
// which is M + 3 launches.  No kernel uses floating-point atomics; every sum has a fixed order, so two fits give the same
// bits.  Every kernel reads the status word first and returns at once when the fit has stopped (a non-finite initial U).
//
// WHY THE HOST DRIVES THE TREE.  The tree is data-dependent: whether a leaf diverges, which leaf becomes the proposal and
// whether a subtree has turned decide what is launched next.  The chunked families enqueue a whole chunk behind a stop word;
// here that would mean enqueueing 2^depth guarded leapfrogs per doubling, up to 1023 x (M + 3) launches per transition, most
// of them empty after the turn.  So the tree, the step-size adaptation and the window schedule are host C++ in this file, and
// the host reads the record ONCE per leapfrog (a copy of 208 bytes through the handle's pinned landing buffer).
// tools/pcca_probe.py measures that wait's share of a leapfrog.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <limits>
#include <vector>

#include "hip_common.h"
#include "abi_guard.h"
#include "fit_driver.h"
#include "reduce.h"
#include "rng_hash.h"
#include "svi_fused.h"

namespace ccz {

namespace {

constexpr int NUTS_MAXD = 10;                  // largest max_tree_depth (numpyro's default)
constexpr int NUTS_NDOT = 2 * NUTS_MAXD + 2;   // two products per closed subtree, two for the whole tree
constexpr int NUTS_NV = 2 + NUTS_NDOT;         // values per workgroup partial: U, kinetic, the dots
constexpr int NUTS_G = 1024;                   // most workgroups of the passes over N
constexpr int NUTS_PT = 1024;                  // threads of k_nuts_finish
constexpr int64_t NUTS_MAX_SLOT_DOUBLES = int64_t(1) << 33;   // 64 GiB of slots

// dual averaging, the windows and the regularised variance: numpyro's defaults (tests/pcca_restatement.py)
constexpr double NUTS_T0 = 10.0, NUTS_KAPPA = 0.75, NUTS_GAMMA = 0.05;
constexpr double NUTS_MAX_DELTA = 1000.0;
constexpr double NUTS_REG_COUNT = 5.0, NUTS_REG_FLOOR = 1e-3;

enum NutsSlot {
  SL_LQ = 0, SL_LP, SL_LG, SL_RQ, SL_RP, SL_RG,      // the tree's ends (left: backwards in time)
  SL_CQ, SL_CG,                                      // the chain's point between transitions; the tree's proposal within one
  SL_SQ, SL_SG,                                      // the proposal of the subtree under construction
  SL_RHO, SL_RSUM,                                   // sum of p over the tree; over the subtree under construction
  SL_MINV, SL_WMEAN, SL_WM2,
  SL_CKPT                                            // + 2 c: p of checkpoint c, + 2 c + 1: the subtree's sum up to and with it
};

struct NutsStatus {
  long long transitions;   // transitions done
  long long bad;           // 0 when the initial potential was not finite, -1 otherwise
  int stopped;
};

struct NutsRecord {
  double U, kinetic, H;
  double dots[NUTS_NDOT];
  long long finite;
};

struct NutsBuf {
  double* slot[SL_CKPT + 2 * NUTS_MAXD];
  double *wpart, *s2part, *zpart;     // the fused kernel's partials (svi_fused.h)
  double* part;                       // NUTS_G x NUTS_NV
  NutsRecord* rec;
  int64_t N, ptot, oS, oZ;
  int n, M, K, nchunk, NS, G;
  double cst;
};

struct NutsSeeds {
  uint64_t s[2 * SVI_MAXV + 1];       // site 2 i: W_i; 2 i + 1: s_i; 2 M: Z
};

// what one fold pass does beside the gradient and the kick
struct NutsLeaf {
  double *q, *p, *g;          // the moving end
  const double* p_other;      // the momentum of the tree's other end
  double eps;                 // signed
  int first;                  // leaf 0 of a subtree: its momentum sum starts here
  int store;                  // checkpoint to write (an even leaf), -1 for none
  int ncheck, cmax;           // subtrees this leaf closes: checkpoints cmax, cmax - 1, .. (ncheck of them)
  int top;                    // the subtree's last leaf: the whole tree's products as well
};

__device__ __forceinline__ void nuts_store_part(const NutsBuf& B, int v, double x, double* sb) {
  const double s = block_sum<4>(x, sb);
  if (threadIdx.x == 0) B.part[blockIdx.x * NUTS_NV + v] = s;
}

// ---- the momentum draw: p = normal / sqrt(minv) into both ends, the chain's point copied to both ends, rho = p ------------
__global__ void __launch_bounds__(256) k_nuts_draw(NutsBuf B, SviViews vw, NutsSeeds sd, const NutsStatus* st) {
  if (fit_stopped(st)) return;
  __shared__ double sb[4];
  const int K = B.K, M = B.M;
  double kin = 0.0;
  for (int64_t e = int64_t(blockIdx.x) * 256 + threadIdx.x; e < B.N; e += int64_t(gridDim.x) * 256) {
    int site;
    int64_t idx;
    if (e < B.oS) {
      const int64_t row = e / K;
      int i = 0;
      while (i + 1 < M && row >= vw.off[i + 1]) ++i;
      site = 2 * i;
      idx = e - vw.off[i] * K;
    } else if (e < B.oZ) {
      const int64_t j = e - B.oS;
      int i = 0;
      while (i + 1 < M && j >= vw.off[i + 1]) ++i;
      site = 2 * i + 1;
      idx = j - vw.off[i];
    } else {
      site = 2 * M;
      idx = e - B.oZ;
    }
    const double mi = B.slot[SL_MINV][e];
    const double p = hash_normal(sd.s[site], uint64_t(idx)) / sqrt(mi);
    const double q = B.slot[SL_CQ][e], g = B.slot[SL_CG][e];
    B.slot[SL_LQ][e] = q; B.slot[SL_RQ][e] = q;
    B.slot[SL_LG][e] = g; B.slot[SL_RG][e] = g;
    B.slot[SL_LP][e] = p; B.slot[SL_RP][e] = p;
    B.slot[SL_RHO][e] = p;
    kin += 0.5 * mi * p * p;
  }
  nuts_store_part(B, 0, 0.0, sb);
  nuts_store_part(B, 1, kin, sb);
}

// ---- the first half kick and the drift -------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) k_nuts_kick(NutsBuf B, NutsLeaf lf, const NutsStatus* st) {
  if (fit_stopped(st)) return;
  const double* __restrict__ minv = B.slot[SL_MINV];
  for (int64_t e = int64_t(blockIdx.x) * 256 + threadIdx.x; e < B.N; e += int64_t(gridDim.x) * 256) {
    const double p = lf.p[e] - (0.5 * lf.eps) * lf.g[e];
    lf.p[e] = p;
    lf.q[e] = lf.q[e] + lf.eps * (minv[e] * p);
  }
}

// ---- the fold, the prior terms, the second half kick, the momentum sums and the partials -----------------------------------
__global__ void __launch_bounds__(256) k_nuts_fold(NutsBuf B, NutsLeaf lf, const NutsStatus* st) {
  if (fit_stopped(st)) return;
  __shared__ double sb[4];
  const double* __restrict__ minv = B.slot[SL_MINV];
  const double* __restrict__ rho = B.slot[SL_RHO];
  double* __restrict__ rsum = B.slot[SL_RSUM];
  const int64_t PK = B.oS, nK = B.N - B.oZ;
  const double dn = double(B.n);
  double u = 0.0, kin = 0.0, dot[NUTS_NDOT];
#pragma unroll
  for (int v = 0; v < NUTS_NDOT; ++v) dot[v] = 0.0;
  for (int64_t e = int64_t(blockIdx.x) * 256 + threadIdx.x; e < B.N; e += int64_t(gridDim.x) * 256) {
    const double qv = lf.q[e];
    double gv;
    if (e < B.oS) {
      double f = 0.0;
      for (int c = 0; c < B.nchunk; ++c) f += B.wpart[int64_t(c) * PK + e];
      gv = qv - f;
      u += 0.5 * qv * qv;
    } else if (e < B.oZ) {
      const int64_t j = e - B.oS;
      double s2 = 0.0;
      for (int c = 0; c < B.nchunk; ++c) s2 += B.s2part[int64_t(c) * B.ptot + j];
      gv = (qv + dn) - s2;
      u += (0.5 * qv * qv + dn * qv) + 0.5 * s2;
    } else {
      const int64_t j = e - B.oZ;
      double f = 0.0;
      for (int s = 0; s < B.NS; ++s) f += B.zpart[int64_t(s) * nK + j];
      gv = qv - f;
      u += 0.5 * qv * qv;
    }
    lf.g[e] = gv;
    const double pn = lf.p[e] - (0.5 * lf.eps) * gv;
    lf.p[e] = pn;
    const double mi = minv[e];
    kin += 0.5 * mi * pn * pn;
    const double rs = lf.first ? pn : rsum[e] + pn;
    rsum[e] = rs;
    if (lf.store >= 0) {
      B.slot[SL_CKPT + 2 * lf.store][e] = pn;
      B.slot[SL_CKPT + 2 * lf.store + 1][e] = rs;
    }
#pragma unroll
    for (int l = 0; l < NUTS_MAXD; ++l)
      if (l < lf.ncheck) {
        const int c = lf.cmax - l;
        const double pc = B.slot[SL_CKPT + 2 * c][e];
        const double sub = (rs - B.slot[SL_CKPT + 2 * c + 1][e]) + pc;
        const double cc = sub - 0.5 * (pc + pn);
        dot[2 * l] += mi * pc * cc;
        dot[2 * l + 1] += mi * pn * cc;
      }
    if (lf.top) {
      const double po = lf.p_other[e];
      const double cc = (rho[e] + rs) - 0.5 * (po + pn);
      dot[2 * NUTS_MAXD] += mi * po * cc;
      dot[2 * NUTS_MAXD + 1] += mi * pn * cc;
    }
  }
  nuts_store_part(B, 0, u, sb);
  nuts_store_part(B, 1, kin, sb);
#pragma unroll
  for (int l = 0; l < NUTS_MAXD; ++l)
    if (l < lf.ncheck) {
      nuts_store_part(B, 2 + 2 * l, dot[2 * l], sb);
      nuts_store_part(B, 3 + 2 * l, dot[2 * l + 1], sb);
    }
  if (lf.top) {
    nuts_store_part(B, 2 + 2 * NUTS_MAXD, dot[2 * NUTS_MAXD], sb);
    nuts_store_part(B, 3 + 2 * NUTS_MAXD, dot[2 * NUTS_MAXD + 1], sb);
  }
}

// one workgroup: value v of the G workgroup partials in a fixed order (32 groups of every 32nd workgroup, then the groups in
// order).  Values no fold pass wrote this time (dots of tests the leaf did not close) are reported as zero.
// mode 0: a leaf; 1: the momentum draw (U is not formed: only the kinetic energy counts); 2: the initial point (a non-finite
// U stops the fit)
__global__ void __launch_bounds__(NUTS_PT) k_nuts_finish(NutsBuf B, int mode, int ncheck, int top, NutsStatus* st) {
  if (fit_stopped(st)) return;
  __shared__ double sw[32][33];
  const int t = threadIdx.x, v = t & 31, grp = t >> 5;
  const bool live = v < 2 || (v - 2 < 2 * ncheck) || (top && v >= 2 + 2 * NUTS_MAXD && v < NUTS_NV);
  double s = 0.0;
  if (live && v < NUTS_NV)
    for (int b = grp; b < B.G; b += 32) s += B.part[b * NUTS_NV + v];
  sw[grp][v] = s;
  __syncthreads();
  if (t < 32) {
    double tot = 0.0;
    for (int gi = 0; gi < 32; ++gi) tot += sw[gi][t];
    sw[0][t] = tot;
  }
  __syncthreads();
  if (t == 0) {
    NutsRecord r;
    r.U = mode == 1 ? 0.0 : sw[0][0] + B.cst;
    r.kinetic = sw[0][1];
    r.H = r.U + r.kinetic;
    for (int d = 0; d < NUTS_NDOT; ++d) r.dots[d] = sw[0][2 + d];
    r.finite = isfinite(r.H) ? 1 : 0;
    *B.rec = r;
    if (mode == 2 && !isfinite(r.U)) {
      st->bad = 0;
      st->stopped = 1;
    }
  }
}

// ---- vector housekeeping, one pass each ----------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) k_nuts_copy2(double* __restrict__ d0, const double* __restrict__ s0, double* __restrict__ d1,
                                                   const double* __restrict__ s1, int64_t count, const NutsStatus* st) {
  if (fit_stopped(st)) return;
  for (int64_t e = int64_t(blockIdx.x) * 256 + threadIdx.x; e < count; e += int64_t(gridDim.x) * 256) {
    d0[e] = s0[e];
    d1[e] = s1[e];
  }
}

__global__ void __launch_bounds__(256) k_nuts_rho_add(double* __restrict__ rho, const double* __restrict__ rsum, int64_t count,
                                                     const NutsStatus* st) {
  if (fit_stopped(st)) return;
  for (int64_t e = int64_t(blockIdx.x) * 256 + threadIdx.x; e < count; e += int64_t(gridDim.x) * 256) rho[e] = rho[e] + rsum[e];
}

// Welford with the new count: d0 = x - mean; mean += d0 / count; M2 += d0 (x - mean)
__global__ void __launch_bounds__(256) k_nuts_welford(double* __restrict__ mean, double* __restrict__ m2, const double* __restrict__ x,
                                                     double count, int64_t len, const NutsStatus* st) {
  if (fit_stopped(st)) return;
  for (int64_t e = int64_t(blockIdx.x) * 256 + threadIdx.x; e < len; e += int64_t(gridDim.x) * 256) {
    const double xv = x[e], d0 = xv - mean[e];
    const double m = mean[e] + d0 / count;
    mean[e] = m;
    m2[e] = m2[e] + d0 * (xv - m);
  }
}

// a window's end: minv = (c / (c + 5)) M2 / (c - 1) + 1e-3 (5 / (c + 5)); the Welford state starts again
__global__ void __launch_bounds__(256) k_nuts_window_end(double* __restrict__ minv, double* __restrict__ mean, double* __restrict__ m2,
                                                        double count, int64_t len, const NutsStatus* st) {
  if (fit_stopped(st)) return;
  for (int64_t e = int64_t(blockIdx.x) * 256 + threadIdx.x; e < len; e += int64_t(gridDim.x) * 256) {
    const double var = m2[e] / (count - 1.0);
    minv[e] = (count / (count + NUTS_REG_COUNT)) * var + NUTS_REG_FLOOR * (NUTS_REG_COUNT / (count + NUTS_REG_COUNT));
    mean[e] = 0.0;
    m2[e] = 0.0;
  }
}

__global__ void __launch_bounds__(256) k_nuts_fill(double* x, int64_t count, double v) {
  for (int64_t e = int64_t(blockIdx.x) * 256 + threadIdx.x; e < count; e += int64_t(gridDim.x) * 256) x[e] = v;
}

// ---- host driver ----------------------------------------------------------------------------------------------------
struct DualAverage {
  double mu = 0.0, x = 0.0, x_avg = 0.0, g_avg = 0.0;
  long long t = 0;
  void init(double m) { mu = m; x = x_avg = g_avg = 0.0; t = 0; }
  void update(double g) {
    t += 1;
    g_avg = (1.0 - 1.0 / (double(t) + NUTS_T0)) * g_avg + g / (double(t) + NUTS_T0);
    x = mu - std::sqrt(double(t)) / NUTS_GAMMA * g_avg;
    const double w = std::pow(double(t), -NUTS_KAPPA);
    x_avg = (1.0 - w) * x_avg + w * x;
  }
};

struct NutsStats {
  std::vector<double> depth, n_leapfrog, accept, diverging, potential, step_size;
};

struct NutsState : FitState<NutsStatus> {
  int64_t n, K;
  uint64_t seed;
  long long num_warmup, num_samples, done = 0;
  int max_depth;
  double target;
  NutsBuf B;
  FusedPlan plan;
  SviViews shape;
  int nslots;
  bool has_init = false;
  // the chain's scalars
  double U = 0.0, eps = 1.0;
  DualAverage da;
  std::vector<std::pair<long long, long long>> windows;
  size_t widx = 0;
  long long wcount = 0;
  NutsStats stats;
};

// the stream of site `site` at transition t (svi.hip's derivation), restated in tests/vbcca_restatement.py
uint64_t nuts_stream(uint64_t seed, uint64_t t, uint64_t site) { return splitmix64(splitmix64(splitmix64(seed) + t) + site); }
// u_j of a transition's tree stream
double nuts_uniform(uint64_t strm, uint64_t j) { return double(splitmix64(strm ^ splitmix64(j)) >> 11) * (1.0 / 9007199254740992.0); }

double log_add_exp(double a, double b) {
  const double hi = std::max(a, b), lo = std::min(a, b);
  return std::isfinite(hi) ? hi + std::log1p(std::exp(lo - hi)) : hi;
}

// Stan's windows as numpyro builds them: inclusive (start, end)
std::vector<std::pair<long long, long long>> window_schedule(long long n) {
  std::vector<std::pair<long long, long long>> out;
  if (n <= 0) return out;
  if (n < 20) {
    out.emplace_back(0, n - 1);
    return out;
  }
  long long init = 75, term = 50, base = 25;
  if (init + base + term > n) {
    init = (long long)(0.15 * double(n));
    term = (long long)(0.1 * double(n));
    base = n - init - term;
  }
  out.emplace_back(0, init - 1);
  const long long end1 = n - term;
  long long size = base, start = init;
  while (start < end1) {
    long long cur = size;
    if (3 * cur <= end1 - start)
      size = 2 * cur;
    else
      cur = end1 - start;
    out.emplace_back(start, start + cur - 1);
    start += cur;
  }
  out.emplace_back(end1, n - 1);
  return out;
}

SviViews make_views(const NutsState& S, const ccz_view* views, const void* const* means) {
  SviViews vw = S.shape;
  fill_views("nuts", vw, views, means, S.p);
  return vw;
}

NutsRecord read_record(ccz_ctx* c, const NutsState& S) {
  NutsRecord r;
  d2h(c, &r, S.B.rec, sizeof(r));
  return r;
}

void copy2(ccz_ctx* c, const NutsState& S, int d0, int s0, int d1, int s1) {
  const NutsBuf& B = S.B;
  hipLaunchKernelGGL(k_nuts_copy2, dim3(B.G), dim3(256), 0, stream(c), B.slot[d0], B.slot[s0], B.slot[d1], B.slot[s1], B.N, S.drv.dev);
  CCZ_LAUNCH_CHECK();
}

// the gradient and the potential at lf.q, the second half kick (M + 2 launches) and the record
NutsRecord gradient_pass(ccz_ctx* c, const NutsState& S, const SviViews& vw, const NutsLeaf& lf, int mode) {
  const NutsBuf& B = S.B;
  for (int i = 0; i < S.M; ++i)
    by_dtype(S.dtype, [&](auto t) {
      launch_fused<decltype(t)>(c, S.plan, vw, i, lf.q, lf.q + B.oS, lf.q + B.oZ, B.wpart, B.s2part, B.zpart, S.drv.dev);
    });
  hipLaunchKernelGGL(k_nuts_fold, dim3(B.G), dim3(256), 0, stream(c), B, lf, S.drv.dev);
  CCZ_LAUNCH_CHECK();
  hipLaunchKernelGGL(k_nuts_finish, dim3(1), dim3(NUTS_PT), 0, stream(c), B, mode, lf.ncheck, lf.top, S.drv.dev);
  CCZ_LAUNCH_CHECK();
  return read_record(c, S);
}

// leaf `leaf` of a doubling at depth `depth` in direction dir (+1: the right end moves forwards, -1: the left end backwards)
NutsRecord leapfrog(ccz_ctx* c, const NutsState& S, const SviViews& vw, int dir, long long leaf, int depth) {
  const NutsBuf& B = S.B;
  NutsLeaf lf;
  const int base = dir > 0 ? SL_RQ : SL_LQ;
  lf.q = B.slot[base]; lf.p = B.slot[base + 1]; lf.g = B.slot[base + 2];
  lf.p_other = B.slot[dir > 0 ? SL_LP : SL_RP];
  lf.eps = double(dir) * S.eps;
  lf.first = leaf == 0;
  const int cmax = __builtin_popcountll((unsigned long long)(leaf >> 1));
  lf.cmax = cmax;
  if (leaf % 2 == 0) {
    lf.store = depth > 0 ? cmax : -1;      // the only leaf of a depth-0 doubling closes nothing and opens nothing
    lf.ncheck = 0;
  } else {
    lf.store = -1;
    int ones = 0;
    for (long long x = leaf; x & 1; x >>= 1) ++ones;
    lf.ncheck = ones;
  }
  lf.top = leaf == (1ll << depth) - 1;
  hipLaunchKernelGGL(k_nuts_kick, dim3(B.G), dim3(256), 0, stream(c), B, lf, S.drv.dev);
  CCZ_LAUNCH_CHECK();
  return gradient_pass(c, S, vw, lf, 0);
}

// the momentum of transition t into both ends, the chain's point with it; returns the kinetic energy
double draw_momentum(ccz_ctx* c, const NutsState& S, long long t) {
  const NutsBuf& B = S.B;
  NutsSeeds sd;
  for (int s = 0; s < 2 * S.M + 1; ++s) sd.s[s] = nuts_stream(S.seed, uint64_t(t), uint64_t(s));
  hipLaunchKernelGGL(k_nuts_draw, dim3(B.G), dim3(256), 0, stream(c), B, S.shape, sd, S.drv.dev);
  CCZ_LAUNCH_CHECK();
  hipLaunchKernelGGL(k_nuts_finish, dim3(1), dim3(NUTS_PT), 0, stream(c), B, 1, 0, 0, S.drv.dev);
  CCZ_LAUNCH_CHECK();
  return read_record(c, S).kinetic;
}

bool turned(const double* d) { return d[0] <= 0.0 || d[1] <= 0.0; }

struct TransitionResult {
  int depth = 0;
  long long n_leapfrog = 0;
  double accept = 0.0;
  bool diverging = false;
};

// one transition of the chain (tests/pcca_restatement.py::transition, the same tests in the same order)
TransitionResult transition(ccz_ctx* c, NutsState& S, const SviViews& vw, long long t) {
  const uint64_t strm = nuts_stream(S.seed, uint64_t(t), uint64_t(2 * S.M + 1));
  uint64_t j = 0;
  const double h0 = S.U + draw_momentum(c, S, t);
  double logw = 0.0, sum_acc = 0.0, prop_u = S.U;
  TransitionResult out;
  while (out.depth < S.max_depth) {
    const int dir = nuts_uniform(strm, j++) < 0.5 ? 1 : -1;
    const int depth = out.depth;
    const int end_q = dir > 0 ? SL_RQ : SL_LQ, end_g = end_q + 2;
    double sub_logw = -std::numeric_limits<double>::infinity(), sub_u = 0.0;
    bool turning = false;
    NutsRecord r;
    for (long long i = 0; i < (1ll << depth); ++i) {
      r = leapfrog(c, S, vw, dir, i, depth);
      out.n_leapfrog += 1;
      double dh = r.H - h0;
      if (std::isnan(dh)) dh = std::numeric_limits<double>::infinity();
      sum_acc += dh <= 0.0 ? 1.0 : std::exp(-dh);
      if (dh > NUTS_MAX_DELTA) {
        out.diverging = true;
        break;
      }
      const double lw = -dh;
      if (i == 0) {
        copy2(c, S, SL_SQ, end_q, SL_SG, end_g);
        sub_logw = lw;
        sub_u = r.U;
      } else {
        const double both = log_add_exp(sub_logw, lw);
        if (nuts_uniform(strm, j++) < std::exp(lw - both)) {
          copy2(c, S, SL_SQ, end_q, SL_SG, end_g);
          sub_u = r.U;
        }
        sub_logw = both;
      }
      if (i & 1) {
        int ones = 0;
        for (long long x = i; x & 1; x >>= 1) ++ones;
        for (int l = 0; l < ones; ++l) turning = turning || turned(r.dots + 2 * l);
      }
      if (turning) break;
    }
    out.depth += 1;
    if (out.diverging || turning) break;
    if (nuts_uniform(strm, j++) < std::exp(std::min(0.0, sub_logw - logw))) {
      copy2(c, S, SL_CQ, SL_SQ, SL_CG, SL_SG);
      prop_u = sub_u;
    }
    logw = log_add_exp(logw, sub_logw);
    hipLaunchKernelGGL(k_nuts_rho_add, dim3(S.B.G), dim3(256), 0, stream(c), S.B.slot[SL_RHO], S.B.slot[SL_RSUM], S.B.N, S.drv.dev);
    CCZ_LAUNCH_CHECK();
    if (turned(r.dots + 2 * NUTS_MAXD)) break;
  }
  S.U = prop_u;
  out.accept = sum_acc / double(std::max<long long>(out.n_leapfrog, 1));
  return out;
}

// the warm-up's bookkeeping after transition t (tests/pcca_restatement.py::sample)
void adapt(ccz_ctx* c, NutsState& S, long long t, double accept) {
  const NutsBuf& B = S.B;
  S.da.update(S.target - accept);
  S.eps = std::exp(t == S.num_warmup - 1 ? S.da.x_avg : S.da.x);
  S.eps = std::max(S.eps, std::numeric_limits<double>::min());
  const bool middle = S.widx > 0 && S.widx + 1 < S.windows.size();
  if (middle) {
    S.wcount += 1;
    hipLaunchKernelGGL(k_nuts_welford, dim3(B.G), dim3(256), 0, stream(c), B.slot[SL_WMEAN], B.slot[SL_WM2], B.slot[SL_CQ], double(S.wcount), B.N,
                       S.drv.dev);
    CCZ_LAUNCH_CHECK();
  }
  if (t == S.windows[S.widx].second) {
    S.widx += 1;
    if (middle) {
      hipLaunchKernelGGL(k_nuts_window_end, dim3(B.G), dim3(256), 0, stream(c), B.slot[SL_MINV], B.slot[SL_WMEAN], B.slot[SL_WM2], double(S.wcount),
                         B.N, S.drv.dev);
      CCZ_LAUNCH_CHECK();
      S.wcount = 0;
      S.da.init(std::log(10.0 * S.eps));
    }
  }
}

NutsState* nuts_create(ccz_ctx* c, int dtype, int M, const int64_t* p, int64_t n, int64_t k, int64_t num_warmup, int64_t num_samples,
                       int max_depth, double target, uint64_t seed) {
  check_dtype("nuts", dtype);
  if (M < 2 || M > SVI_MAXV) fail(CCZ_EUNSUP, "nuts: 2 to %d views are supported, got %d", SVI_MAXV, M);
  if (k < 1 || k > SVI_MAXK) fail(CCZ_EUNSUP, "nuts: 1 to %d latent dimensions are supported, got %lld", SVI_MAXK, (long long)k);
  if (max_depth < 1 || max_depth > NUTS_MAXD) fail(CCZ_EUNSUP, "nuts: max_tree_depth must be 1 to %d, got %d", NUTS_MAXD, max_depth);
  if (!p || n < 2 || n > (int64_t(1) << 30) || num_warmup < 0 || num_samples < 0 || num_warmup + num_samples < 1 ||
      num_warmup + num_samples > (int64_t(1) << 30) || !(target > 0.0 && target < 1.0))
    fail(CCZ_EINVAL, "nuts: bad argument");
  check_no_empty_view("nuts", M, p);
  return new_state<NutsState>(c, [&](NutsState& S) {
    S.dtype = dtype; S.M = M; S.n = n; S.K = k; S.chunk = 1; S.seed = seed;
    S.num_warmup = num_warmup; S.num_samples = num_samples; S.max_depth = max_depth; S.target = target;
    S.p.assign(p, p + M);
    NutsBuf& B = S.B;
    memset(&B, 0, sizeof(B));
    memset(&S.shape, 0, sizeof(S.shape));
    fused_plan("nuts", M, p, n, k, S.shape, S.plan);
    B.n = int(n); B.M = M; B.K = int(k);
    B.ptot = S.plan.ptot; B.nchunk = S.plan.nchunk; B.NS = S.plan.NS;
    B.oS = B.ptot * k; B.oZ = B.oS + B.ptot;
    B.N = B.oZ + n * k;
    S.nslots = SL_CKPT + 2 * max_depth;
    if (int64_t(S.nslots) * B.N > NUTS_MAX_SLOT_DOUBLES)
      fail(CCZ_EUNSUP, "nuts: %d slots of %lld doubles exceed %lld GiB; lower max_tree_depth or the problem's size", S.nslots,
           (long long)B.N, (long long)(NUTS_MAX_SLOT_DOUBLES >> 27));
    B.G = int(std::max<int64_t>(1, std::min<int64_t>(NUTS_G, (B.N + 255) / 256)));
    // every normalising constant: log(2 pi) / 2 per prior and likelihood term
    B.cst = 0.5 * std::log(2.0 * M_PI) * (double(B.N) + double(n) * double(B.ptot));
    for (int s = 0; s < S.nslots; ++s) B.slot[s] = S.get(c, size_t(B.N));
    B.wpart = S.get(c, size_t(B.nchunk) * B.ptot * k);
    B.s2part = S.get(c, size_t(B.nchunk) * B.ptot);
    B.zpart = S.get(c, size_t(B.NS) * n * k);
    B.part = S.get(c, size_t(NUTS_G) * NUTS_NV);
    B.rec = S.get<NutsRecord>(c, 1);
    S.windows = window_schedule(num_warmup);
    S.drv.create(c);
  });
}

void fill(ccz_ctx* c, double* x, int64_t count, double v) {
  const int g = int(std::max<int64_t>(1, std::min<int64_t>(4096, (count + 255) / 256)));
  hipLaunchKernelGGL(k_nuts_fill, dim3(g), dim3(256), 0, stream(c), x, count, v);
  CCZ_LAUNCH_CHECK();
}

void record_out(const NutsRecord& r, double* out) {
  out[0] = r.U; out[1] = r.kinetic; out[2] = r.H;
  for (int d = 0; d < NUTS_NDOT; ++d) out[3 + d] = r.dots[d];
  out[3 + NUTS_NDOT] = double(r.finite);
}

NutsState& checked(void* state) {
  NutsState& S = *as_state<NutsState>("nuts", state);
  if (!S.has_init) fail(CCZ_EINVAL, "nuts: ccz_nuts_set_init has not been called");
  return S;
}

}  // namespace
}  // namespace ccz

extern "C" {

int ccz_nuts_create(ccz_handle h, int dtype, int n_views, const int64_t* p, int64_t n_rows, int64_t k, int64_t num_warmup,
                    int64_t num_samples, int max_tree_depth, double target_accept_prob, uint64_t seed, void** state_out) {
  CCZ_GUARD(h, {
    if (!state_out) ccz::fail(CCZ_EINVAL, "null argument");
    *state_out = nullptr;
    *state_out = ccz::nuts_create(h, dtype, n_views, p, n_rows, k, num_warmup, num_samples, max_tree_depth, target_accept_prob, seed);
  })
}

int ccz_nuts_destroy(ccz_handle h, void* state) {
  CCZ_GUARD(h, {
    if (state) ccz::free_state(h, static_cast<ccz::NutsState*>(state));
  })
}

int ccz_nuts_set_init(ccz_handle h, void* state, const ccz_view* views, const void* const* means_dev, const double* q_host,
                      double* potential_out) {
  CCZ_GUARD(h, {
    ccz::NutsState& S = *ccz::as_state<ccz::NutsState>("nuts", state);
    const ccz::NutsBuf& B = S.B;
    if (!q_host) ccz::fail(CCZ_EINVAL, "nuts: null initial point");
    const ccz::SviViews vw = ccz::make_views(S, views, means_dev);
    S.restart(h);
    ccz::NutsStatus st;
    memset(&st, 0, sizeof(st));
    st.bad = -1;
    ccz::h2d(h, S.drv.dev, &st, sizeof(st));
    for (int s = 0; s < S.nslots; ++s) ccz::zero(h, B.slot[s], size_t(B.N) * 8);
    ccz::fill(h, B.slot[ccz::SL_MINV], B.N, 1.0);
    ccz::h2d(h, B.slot[ccz::SL_LQ], q_host, size_t(B.N) * 8);
    // U and g at the point: a fold pass with a zero momentum and a zero step
    ccz::NutsLeaf lf;
    lf.q = B.slot[ccz::SL_LQ]; lf.p = B.slot[ccz::SL_LP]; lf.g = B.slot[ccz::SL_LG];
    lf.p_other = B.slot[ccz::SL_RP];
    lf.eps = 0.0; lf.first = 1; lf.store = -1; lf.ncheck = 0; lf.cmax = 0; lf.top = 0;
    const ccz::NutsRecord r = ccz::gradient_pass(h, S, vw, lf, 2);
    ccz::copy2(h, S, ccz::SL_CQ, ccz::SL_LQ, ccz::SL_CG, ccz::SL_LG);
    ccz::d2h(h, &st, S.drv.dev, sizeof(st));
    S.U = r.U;
    S.eps = 1.0;
    S.da.init(std::log(10.0 * S.eps));
    S.widx = 0;
    S.wcount = 0;
    S.done = 0;
    S.stats = ccz::NutsStats();
    S.has_init = true;
    if (potential_out) *potential_out = st.stopped ? std::numeric_limits<double>::quiet_NaN() : r.U;
  })
}

int ccz_nuts_set_adapt(ccz_handle h, void* state, double step_size, const double* minv_host) {
  CCZ_GUARD(h, {
    ccz::NutsState& S = ccz::checked(state);
    if (!(step_size > 0.0) || !std::isfinite(step_size)) ccz::fail(CCZ_EINVAL, "nuts: the step size must be positive");
    S.eps = step_size;
    S.da.init(std::log(10.0 * S.eps));
    if (minv_host) ccz::h2d(h, S.B.slot[ccz::SL_MINV], minv_host, size_t(S.B.N) * 8);
  })
}

int ccz_nuts_leapfrog(ccz_handle h, void* state, const ccz_view* views, const void* const* means_dev, int64_t transition, int begin,
                      int direction, int64_t leaf, int depth, double* record_host) {
  CCZ_GUARD(h, {
    ccz::NutsState& S = ccz::checked(state);
    if (transition < 0 || (direction != 1 && direction != -1) || depth < 0 || depth > S.max_depth || leaf < 0 ||
        leaf >= (int64_t(1) << depth) || !record_host)
      ccz::fail(CCZ_EINVAL, "nuts: bad argument");
    const ccz::SviViews vw = ccz::make_views(S, views, means_dev);
    double k0 = 0.0;
    if (begin) k0 = ccz::draw_momentum(h, S, transition);
    const ccz::NutsRecord r = ccz::leapfrog(h, S, vw, direction, leaf, depth);
    ccz::record_out(r, record_host);
    record_host[4 + ccz::NUTS_NDOT] = k0;
  })
}

int ccz_nuts_run(ccz_handle h, void* state, const ccz_view* views, const void* const* means_dev, int64_t n_transitions,
                 double* draws_host) {
  CCZ_GUARD(h, {
    ccz::NutsState& S = ccz::checked(state);
    const ccz::NutsBuf& B = S.B;
    const long long total = S.num_warmup + S.num_samples;
    if (n_transitions < 0 || S.done + n_transitions > total) ccz::fail(CCZ_EINVAL, "nuts: more transitions than the fit state was created for");
    const ccz::SviViews vw = ccz::make_views(S, views, means_dev);
    ccz::NutsStatus st;
    ccz::d2h(h, &st, S.drv.dev, sizeof(st));
    if (st.stopped) ccz::fail(CCZ_EINVAL, "nuts: the fit has stopped (the initial potential is not finite)");
    for (int64_t s = 0; s < n_transitions; ++s) {
      const long long t = S.done;
      const double eps = S.eps;
      const ccz::TransitionResult tr = ccz::transition(h, S, vw, t);
      S.stats.depth.push_back(tr.depth);
      S.stats.n_leapfrog.push_back(double(tr.n_leapfrog));
      S.stats.accept.push_back(tr.accept);
      S.stats.diverging.push_back(tr.diverging ? 1.0 : 0.0);
      S.stats.potential.push_back(S.U);
      S.stats.step_size.push_back(eps);
      if (t < S.num_warmup) {
        ccz::adapt(h, S, t, tr.accept);
      } else if (draws_host) {
        ccz::d2h(h, draws_host + (t - S.num_warmup) * B.N, B.slot[ccz::SL_CQ], size_t(B.N) * 8);
      }
      S.done = t + 1;
    }
    st.transitions = S.done;
    ccz::h2d(h, S.drv.dev, &st, sizeof(st));
    ccz::sync(h);
  })
}

int ccz_nuts_status(ccz_handle h, void* state, int64_t* transitions, int* stopped, int64_t* bad) {
  CCZ_GUARD(h, {
    ccz::NutsState& S = ccz::checked(state);
    ccz::NutsStatus st;
    ccz::d2h(h, &st, S.drv.dev, sizeof(st));
    if (transitions) *transitions = S.done;
    if (stopped) *stopped = st.stopped;
    if (bad) *bad = st.bad;
  })
}

int ccz_nuts_peek(ccz_handle h, void* state, int what, double* out_host) {
  CCZ_GUARD(h, {
    ccz::NutsState& S = what == CCZ_NUTS_PEEK_PLAN ? *ccz::as_state<ccz::NutsState>("nuts", state) : ccz::checked(state);
    const ccz::NutsBuf& B = S.B;
    if (!out_host) ccz::fail(CCZ_EINVAL, "nuts: bad argument");
    if (what >= 0 && what < S.nslots) {
      ccz::d2h(h, out_host, B.slot[what], size_t(B.N) * 8);
    } else if (what == CCZ_NUTS_PEEK_PLAN) {
      ccz::sync(h);
      out_host[0] = B.nchunk; out_host[1] = S.plan.rc; out_host[2] = B.NS; out_host[3] = B.G; out_host[4] = S.nslots;
      for (int i = 0; i < S.M; ++i) out_host[5 + i] = S.shape.ns[i];
    } else if (what == CCZ_NUTS_PEEK_RECORD) {
      ccz::record_out(ccz::read_record(h, S), out_host);
    } else if (what == CCZ_NUTS_PEEK_SCALARS) {
      ccz::sync(h);
      out_host[0] = S.U; out_host[1] = S.eps; out_host[2] = double(S.wcount); out_host[3] = double(S.widx);
    } else {
      ccz::fail(CCZ_EINVAL, "nuts: unknown buffer %d", what);
    }
  })
}

int ccz_nuts_get_stats(ccz_handle h, void* state, double* stats_host, double* step_size, double* minv_host) {
  CCZ_GUARD(h, {
    ccz::NutsState& S = ccz::checked(state);
    const size_t T = S.stats.depth.size();
    if (stats_host) {
      const std::vector<double>* cols[] = {&S.stats.depth, &S.stats.n_leapfrog, &S.stats.accept, &S.stats.diverging, &S.stats.potential,
                                           &S.stats.step_size};
      for (int a = 0; a < 6; ++a)
        for (size_t t = 0; t < T; ++t) stats_host[a * T + t] = (*cols[a])[t];
    }
    if (step_size) *step_size = S.eps;
    if (minv_host) ccz::d2h(h, minv_host, S.B.slot[ccz::SL_MINV], size_t(S.B.N) * 8);
  })
}

}  // extern "C"
