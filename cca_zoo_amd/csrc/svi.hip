// VariationalBayesCCA: whole steps of mean-field stochastic variational inference on the device.
//
// The algorithm is written down in include/ccz.h (the ccz_svi_* section) and restated in NumPy in tests/vbcca_restatement.py.
// All variational parameters lie in one flat vector of N = K + ptot K + ptot + n K doubles:
//   [ a (K) | W of all views back to back (ptot x K, row-major) | s of all views (ptot) | Z (n x K) ]
// and loc, rho, the four Adam moments, theta, eps and the gradient share that layout.  One step t, for M views:
//   k_svi_draw              theta = loc + softplus(rho) eps, eps = hash_normal(stream(seed, t, site), index in the site)
//   per view i:
//     k_svi_fused_*         ONE read of X_i (svi_fused.h, shared with nuts.hip): the row-chunk partials of D' Z and of
//                           sum R^2 exp(-2 s), the strip partials of D W_i
//   k_svi_adam              W, Z and s sites: the partials folded in index order, the prior terms, d loc / d rho, Adam; per-workgroup
//                           partial sums of the loss terms and of the column sums of W^2
//   k_svi_finish            one workgroup: the a site (its gradient needs sum W^2), loss[t], the non-finite stop
// which is 3 + M launches.  No kernel uses floating-point atomics; every sum has a fixed order, so two fits give the same bits
// whatever the chunk length.  Every kernel reads the status word first and returns at once when the fit has stopped.
//
// Precision: x - mu is rounded in the views' precision, then widened; every product and sum is fp64.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <vector>

#include "hip_common.h"
#include "abi_guard.h"
#include "fit_driver.h"
#include "reduce.h"
#include "rng_hash.h"
#include "row_load.h"
#include "svi_fused.h"

namespace ccz {

namespace {

constexpr int SVI_G = 1024;             // most workgroups of k_svi_adam
constexpr int SVI_PT = 1024;            // threads of k_svi_finish

constexpr double SVI_A0 = 1e-3, SVI_B0 = 1e-3;       // cca_zoo/probabilistic/_vbcca.py:16-17
constexpr double SVI_B1 = 0.9, SVI_B2 = 0.999, SVI_ADAM_EPS = 1e-8;
constexpr double SVI_INIT_SCALE = 0.1;

struct SviStatus {
  long long steps;        // steps done
  long long bad_step;     // the step whose loss was not finite, -1 when none
  int stopped;
};

struct SviSeeds {
  uint64_t s[2 * SVI_MAXV + 2];    // site 0: a; 1 + 2 i: W_i; 2 + 2 i: s_i; 1 + 2 M: Z
};

struct SviBuf {
  double *loc, *rho, *m1, *v1, *m2, *v2, *theta, *eps, *grad;   // N each
  double* wpart;      // nchunk x ptot x K: row-chunk partial sums of D' Z
  double* s2part;     // nchunk x ptot: row-chunk partial sums of R^2 exp(-2 s)
  double* zpart;      // NS x n x K: strip partial sums of D W
  double* losspart;   // SVI_G
  double* w2part;     // SVI_G x 32
  double* loss;       // total steps
  int64_t N, ptot, oW, oS, oZ;
  int n, M, K, nchunk, rc, NS, gadam;
  long long total;
  double lr, cst;
};

__device__ __forceinline__ double svi_softplus(double r) { return r > 0.0 ? r + log1p(exp(-r)) : log1p(exp(r)); }
__device__ __forceinline__ double svi_sigmoid(double r) { return 1.0 / (1.0 + exp(-r)); }

// ---- theta and eps ------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) k_svi_draw(SviBuf B, SviViews vw, SviSeeds sd, const SviStatus* st) {
  if (fit_stopped(st)) return;
  const int K = B.K, M = B.M;
  for (int64_t e = int64_t(blockIdx.x) * 256 + threadIdx.x; e < B.N; e += int64_t(gridDim.x) * 256) {
    int site;
    int64_t idx;
    if (e < B.oW) {
      site = 0;
      idx = e;
    } else if (e < B.oS) {
      const int64_t row = (e - B.oW) / K;
      int i = 0;
      while (i + 1 < M && row >= vw.off[i + 1]) ++i;
      site = 1 + 2 * i;
      idx = e - B.oW - vw.off[i] * K;
    } else if (e < B.oZ) {
      const int64_t j = e - B.oS;
      int i = 0;
      while (i + 1 < M && j >= vw.off[i + 1]) ++i;
      site = 2 + 2 * i;
      idx = j - vw.off[i];
    } else {
      site = 1 + 2 * M;
      idx = e - B.oZ;
    }
    const double ep = hash_normal(sd.s[site], uint64_t(idx));
    B.eps[e] = ep;
    B.theta[e] = B.loc[e] + svi_softplus(B.rho[e]) * ep;
  }
}

// ---- the folds, the prior terms and Adam -------------------------------------------------------------------------------------
struct SviAdam {
  double lr, c1, c2;     // the bias corrections 1 - b1^(t+1), 1 - b2^(t+1)
};

// element e with d ELBO / d theta = g: d loc = g, d rho = (g eps + 1 / scale) sigmoid(rho); Adam on the loss (minus the ELBO).
// Returns the element's share of the entropy without its constant: log scale + eps^2 / 2.
__device__ __forceinline__ double svi_update(const SviBuf& B, const SviAdam& ad, int64_t e, double g) {
  const double ep = B.eps[e], rho = B.rho[e];
  const double scale = svi_softplus(rho);
  B.grad[e] = g;
  const double gl = -g, gr = -((g * ep + 1.0 / scale) * svi_sigmoid(rho));
  const double m1 = SVI_B1 * B.m1[e] + (1.0 - SVI_B1) * gl, v1 = SVI_B2 * B.v1[e] + (1.0 - SVI_B2) * (gl * gl);
  const double m2 = SVI_B1 * B.m2[e] + (1.0 - SVI_B1) * gr, v2 = SVI_B2 * B.v2[e] + (1.0 - SVI_B2) * (gr * gr);
  B.m1[e] = m1; B.v1[e] = v1; B.m2[e] = m2; B.v2[e] = v2;
  B.loc[e] = B.loc[e] - ad.lr * (m1 / ad.c1) / (sqrt(v1 / ad.c2) + SVI_ADAM_EPS);
  B.rho[e] = rho - ad.lr * (m2 / ad.c1) / (sqrt(v2 / ad.c2) + SVI_ADAM_EPS);
  return log(scale) + 0.5 * ep * ep;
}

// grid gadam <= SVI_G workgroups of 256 threads.  W and Z rows: thread (row t / KP, column t % KP), KP the power of two >= K
__global__ void __launch_bounds__(256) k_svi_adam(SviBuf B, SviAdam ad, const SviStatus* st) {
  if (fit_stopped(st)) return;
  __shared__ double sh[256];
  __shared__ double sb[4];
  const int K = B.K, t = threadIdx.x, n = B.n;
  int KP = 1;
  while (KP < K) KP <<= 1;
  const int RP = 256 / KP, col = t % KP, rl = t / KP;
  double lacc = 0.0, w2 = 0.0;
  if (col < K) {
    const double alpha = exp(B.theta[col]);
    for (int64_t row = int64_t(blockIdx.x) * RP + rl; row < B.ptot; row += int64_t(gridDim.x) * RP) {
      const int64_t e = B.oW + row * K + col;
      double g = 0.0;
      for (int c = 0; c < B.nchunk; ++c) g += B.wpart[(int64_t(c) * B.ptot + row) * K + col];
      const double th = B.theta[e];
      g -= alpha * th;
      w2 += th * th;
      lacc += svi_update(B, ad, e, g);
    }
    for (int64_t row = int64_t(blockIdx.x) * RP + rl; row < n; row += int64_t(gridDim.x) * RP) {
      const int64_t e = B.oZ + row * K + col;
      double g = 0.0;
      for (int s = 0; s < B.NS; ++s) g += B.zpart[(int64_t(s) * n + row) * K + col];
      const double th = B.theta[e];
      g -= th;
      lacc += -0.5 * th * th;
      lacc += svi_update(B, ad, e, g);
    }
  }
  for (int64_t j = int64_t(blockIdx.x) * 256 + t; j < B.ptot; j += int64_t(gridDim.x) * 256) {
    const int64_t e = B.oS + j;
    double s2 = 0.0;
    for (int c = 0; c < B.nchunk; ++c) s2 += B.s2part[int64_t(c) * B.ptot + j];
    const double th = B.theta[e];
    lacc += (-0.5 * s2 - double(n) * th) - 0.5 * th * th;
    lacc += svi_update(B, ad, e, (s2 - double(n)) - th);
  }
  sh[t] = w2;
  __syncthreads();
  if (t < 32) {
    double s = 0.0;
    if (t < K)
      for (int r = 0; r < RP; ++r) s += sh[r * KP + t];
    B.w2part[blockIdx.x * 32 + t] = s;
  }
  lacc = block_sum<4>(lacc, sb);
  if (t == 0) B.losspart[blockIdx.x] = lacc;
}

// one workgroup: sum W^2 per column and the loss partials in a fixed order, the a site, loss[t], the stop
__global__ void __launch_bounds__(SVI_PT) k_svi_finish(SviBuf B, SviAdam ad, long long step, SviStatus* st) {
  if (fit_stopped(st)) return;
  __shared__ double sw[32][33];
  __shared__ double sa[32];
  __shared__ double sb[SVI_PT / 64];
  const int K = B.K, t = threadIdx.x, G = B.gadam;
  double part = 0.0;
  for (int b = t; b < G; b += SVI_PT) part += B.losspart[b];
  const double tot = block_sum<SVI_PT / 64>(part, sb);
  {
    const int a = t & 31, grp = t >> 5;
    double s = 0.0;
    for (int b = grp; b < G; b += 32) s += B.w2part[b * 32 + a];
    sw[grp][a] = s;
  }
  __syncthreads();
  if (t < 32) {
    double la = 0.0;
    if (t < K) {
      double S = 0.0;
      for (int grp = 0; grp < 32; ++grp) S += sw[grp][t];
      const double th = B.theta[t], alpha = exp(th), P = double(B.ptot);
      const double g = ((SVI_A0 - SVI_B0 * alpha) + 0.5 * P) - 0.5 * alpha * S;
      la = (((SVI_A0 - 1.0) * th - SVI_B0 * alpha) + th) + (0.5 * P * th - 0.5 * alpha * S);
      la += svi_update(B, ad, t, g);
    }
    sa[t] = la;
  }
  __syncthreads();
  if (t == 0) {
    double elbo = tot;
    for (int a = 0; a < K; ++a) elbo += sa[a];
    elbo += B.cst;
    const double loss = -elbo;
    B.loss[step] = loss;
    st->steps = step + 1;
    if (!isfinite(loss)) {
      st->bad_step = step;
      st->stopped = 1;
    } else if (step + 1 >= B.total) {
      st->stopped = 1;
    }
  }
}

__global__ void __launch_bounds__(256) k_svi_fill(double* x, int64_t count, double v) {
  for (int64_t e = int64_t(blockIdx.x) * 256 + threadIdx.x; e < count; e += int64_t(gridDim.x) * 256) x[e] = v;
}

// ---- sum_j wt_j sum_rows fl(x - mu)^2 -------------------------------------------------------------------------------------
template <typename T>
__global__ void __launch_bounds__(256) k_svi_colsq(const T* __restrict__ X, const T* __restrict__ mu, int64_t ld, int64_t p, int n, int rc,
                                                  double* __restrict__ part) {
  const int64_t f = int64_t(blockIdx.x) * 256 + threadIdx.x;
  if (f >= p) return;
  const int r0 = blockIdx.y * rc, r1 = min(n, r0 + rc);
  const T m = mu ? mu[f] : T(0);
  double s2 = 0.0;
  for (int r = r0; r < r1; ++r) {
    const double xc = double(T(X[int64_t(r) * ld + f] - m));
    s2 += xc * xc;
  }
  part[int64_t(blockIdx.y) * p + f] = s2;
}

__global__ void __launch_bounds__(SVI_PT) k_svi_colsq_fold(const double* __restrict__ part, int sc, int64_t p, const double* __restrict__ wt,
                                                          double* __restrict__ out) {
  __shared__ double sb[SVI_PT / 64];
  double tot = 0.0;
  for (int64_t f = threadIdx.x; f < p; f += SVI_PT) {
    double s2 = 0.0;
    for (int c = 0; c < sc; ++c) s2 += part[int64_t(c) * p + f];
    tot += wt[f] * s2;
  }
  tot = block_sum<SVI_PT / 64>(tot, sb);
  if (threadIdx.x == 0) *out = tot;
}

// ---- host driver ----------------------------------------------------------------------------------------------------
struct SviState : FitState<SviStatus> {
  int64_t n, K;
  uint64_t seed;
  long long done = 0;       // steps enqueued
  SviBuf B;
  SviViews shape;
  bool has_init = false;
};

// the stream of site `site` at step t: one definition, restated in tests/vbcca_restatement.py
uint64_t svi_stream(uint64_t seed, uint64_t t, uint64_t site) { return splitmix64(splitmix64(splitmix64(seed) + t) + site); }

SviViews make_views(const SviState& S, const ccz_view* views, const void* const* means) {
  SviViews vw = S.shape;
  fill_views("svi", vw, views, means, S.p);
  return vw;
}

void enqueue_step(ccz_ctx* c, const SviState& S, const SviViews& vw, long long step) {
  const SviBuf& B = S.B;
  SviSeeds sd;
  for (int s = 0; s < 2 * S.M + 2; ++s) sd.s[s] = svi_stream(S.seed, uint64_t(step), uint64_t(s));
  SviAdam ad;
  ad.lr = B.lr;
  ad.c1 = 1.0 - std::pow(SVI_B1, double(step + 1));
  ad.c2 = 1.0 - std::pow(SVI_B2, double(step + 1));
  const int gd = int(std::max<int64_t>(1, std::min<int64_t>(4096, (B.N + 1023) / 1024)));
  hipLaunchKernelGGL(k_svi_draw, dim3(gd), dim3(256), 0, stream(c), B, vw, sd, S.drv.dev);
  CCZ_LAUNCH_CHECK();
  const FusedPlan P{B.ptot, B.n, B.K, B.nchunk, B.rc, B.NS};
  for (int i = 0; i < S.M; ++i)
    by_dtype(S.dtype, [&](auto t) {
      launch_fused<decltype(t)>(c, P, vw, i, B.theta + B.oW, B.theta + B.oS, B.theta + B.oZ, B.wpart, B.s2part, B.zpart, S.drv.dev);
    });
  hipLaunchKernelGGL(k_svi_adam, dim3(B.gadam), dim3(256), 0, stream(c), B, ad, S.drv.dev);
  CCZ_LAUNCH_CHECK();
  hipLaunchKernelGGL(k_svi_finish, dim3(1), dim3(SVI_PT), 0, stream(c), B, ad, step, S.drv.dev);
  CCZ_LAUNCH_CHECK();
}

SviState* svi_create(ccz_ctx* c, int dtype, int M, const int64_t* p, int64_t n, int64_t k, int64_t num_steps, double lr, uint64_t seed,
                     int64_t chunk) {
  check_dtype("svi", dtype);
  if (M < 2 || M > SVI_MAXV) fail(CCZ_EUNSUP, "svi: 2 to %d views are supported, got %d", SVI_MAXV, M);
  if (k < 1 || k > SVI_MAXK) fail(CCZ_EUNSUP, "svi: 1 to %d latent dimensions are supported, got %lld", SVI_MAXK, (long long)k);
  if (!p || n < 2 || n > (int64_t(1) << 30) || num_steps < 1 || num_steps > (int64_t(1) << 30) || chunk < 1 || !(lr > 0.0))
    fail(CCZ_EINVAL, "svi: bad argument");
  check_no_empty_view("svi", M, p);
  return new_state<SviState>(c, [&](SviState& S) {
    S.dtype = dtype; S.M = M; S.n = n; S.K = k; S.chunk = chunk; S.seed = seed;
    S.p.assign(p, p + M);
    SviBuf& B = S.B;
    memset(&B, 0, sizeof(B));
    memset(&S.shape, 0, sizeof(S.shape));
    B.n = int(n); B.M = M; B.K = int(k); B.total = num_steps; B.lr = lr;
    FusedPlan P;
    fused_plan("svi", M, p, n, k, S.shape, P);
    B.ptot = P.ptot; B.NS = P.NS; B.rc = P.rc; B.nchunk = P.nchunk;
    B.N = k + B.ptot * k + B.ptot + n * k;
    B.oW = k; B.oS = k + B.ptot * k; B.oZ = B.oS + B.ptot;
    B.gadam = int(std::max<int64_t>(1, std::min<int64_t>(SVI_G, (std::max<int64_t>(B.ptot, n) * k + 255) / 256)));
    // every normalising constant: the Gamma prior's, -log(2 pi) / 2 per prior and likelihood term, +log(2 pi) / 2 per entropy term
    B.cst = double(k) * (SVI_A0 * std::log(SVI_B0) - std::lgamma(SVI_A0)) +
            0.5 * std::log(2.0 * M_PI) * (double(k) - double(n) * double(B.ptot));
    double** all[] = {&B.loc, &B.rho, &B.m1, &B.v1, &B.m2, &B.v2, &B.theta, &B.eps, &B.grad};
    for (double** b : all) *b = S.get(c, size_t(B.N));
    B.wpart = S.get(c, size_t(B.nchunk) * B.ptot * k);
    B.s2part = S.get(c, size_t(B.nchunk) * B.ptot);
    B.zpart = S.get(c, size_t(B.NS) * n * k);
    B.losspart = S.get(c, SVI_G);
    B.w2part = S.get(c, size_t(SVI_G) * 32);
    B.loss = S.get(c, size_t(num_steps));
    S.drv.create(c);
  });
}

SviStatus read_status(ccz_ctx* c, const SviState& S) {
  SviStatus st;
  d2h(c, &st, S.drv.dev, sizeof(st));
  return st;
}

void fill(ccz_ctx* c, double* x, int64_t count, double v) {
  const int g = int(std::max<int64_t>(1, std::min<int64_t>(4096, (count + 255) / 256)));
  hipLaunchKernelGGL(k_svi_fill, dim3(g), dim3(256), 0, stream(c), x, count, v);
  CCZ_LAUNCH_CHECK();
}

}  // namespace
}  // namespace ccz

extern "C" {

int ccz_svi_create(ccz_handle h, int dtype, int n_views, const int64_t* p, int64_t n_rows, int64_t k, int64_t num_steps,
                   double learning_rate, uint64_t seed, int64_t chunk_steps, void** state_out) {
  CCZ_GUARD(h, {
    if (!state_out) ccz::fail(CCZ_EINVAL, "null argument");
    *state_out = nullptr;
    *state_out = ccz::svi_create(h, dtype, n_views, p, n_rows, k, num_steps, learning_rate, seed, chunk_steps);
  })
}

int ccz_svi_destroy(ccz_handle h, void* state) {
  CCZ_GUARD(h, {
    if (state) ccz::free_state(h, static_cast<ccz::SviState*>(state));
  })
}

int ccz_svi_set_init(ccz_handle h, void* state, const double* loc_host) {
  CCZ_GUARD(h, {
    ccz::SviState& S = *ccz::as_state<ccz::SviState>("svi", state);
    const ccz::SviBuf& B = S.B;
    if (!loc_host) ccz::fail(CCZ_EINVAL, "svi: null initial loc");
    S.restart(h);
    ccz::h2d(h, B.loc, loc_host, size_t(B.N) * 8);
    ccz::fill(h, B.rho, B.N, std::log(std::expm1(ccz::SVI_INIT_SCALE)));
    double* zeroed[] = {B.m1, B.v1, B.m2, B.v2, B.theta, B.eps, B.grad};
    for (double* b : zeroed) ccz::zero(h, b, size_t(B.N) * 8);
    ccz::zero(h, B.loss, size_t(B.total) * 8);
    ccz::SviStatus st;
    memset(&st, 0, sizeof(st));
    st.bad_step = -1;
    ccz::h2d(h, S.drv.dev, &st, sizeof(st));
    S.done = 0;
    S.has_init = true;
  })
}

int ccz_svi_steps(ccz_handle h, void* state, const ccz_view* views, const void* const* means_dev, int64_t n_steps, int64_t* steps_known,
                  int* stopped_known) {
  CCZ_GUARD(h, {
    ccz::SviState& S = *ccz::as_state<ccz::SviState>("svi", state);
    if (!S.has_init) ccz::fail(CCZ_EINVAL, "svi: ccz_svi_set_init has not been called");
    if (n_steps > 0 && S.done + n_steps > S.B.total) ccz::fail(CCZ_EINVAL, "svi: more steps than the fit state was created for");
    const long long first = S.done;
    ccz::run_chunk(h, "svi", "n_steps", S, n_steps, steps_known, stopped_known, &ccz::SviStatus::steps,
                   [&] { return ccz::make_views(S, views, means_dev); },
                   [&](const ccz::SviViews& vw, int64_t t) { ccz::enqueue_step(h, S, vw, first + t); });
    S.done = first + n_steps;
  })
}

int ccz_svi_status(ccz_handle h, void* state, int64_t* steps, int* stopped, int64_t* bad_step) {
  CCZ_GUARD(h, {
    ccz::SviState& S = *ccz::as_state<ccz::SviState>("svi", state);
    if (!S.has_init) ccz::fail(CCZ_EINVAL, "svi: ccz_svi_set_init has not been called");
    const ccz::SviStatus st = ccz::read_status(h, S);
    if (steps) *steps = st.steps;
    if (stopped) *stopped = st.stopped;
    if (bad_step) *bad_step = st.bad_step;
  })
}

int ccz_svi_peek(ccz_handle h, void* state, int what, double* out_host) {
  CCZ_GUARD(h, {
    ccz::SviState& S = *ccz::as_state<ccz::SviState>("svi", state);
    const ccz::SviBuf& B = S.B;
    if (!S.has_init) ccz::fail(CCZ_EINVAL, "svi: ccz_svi_set_init has not been called");
    if (!out_host) ccz::fail(CCZ_EINVAL, "svi: bad argument");
    const double* flat[] = {B.loc, B.rho, B.m1, B.v1, B.m2, B.v2, B.theta, B.eps, B.grad};
    if (what >= 0 && what <= CCZ_SVI_PEEK_GRAD) {
      ccz::d2h(h, out_host, flat[what], size_t(B.N) * 8);
    } else if (what == CCZ_SVI_PEEK_LOSS) {
      ccz::d2h(h, out_host, B.loss, size_t(B.total) * 8);
    } else if (what == CCZ_SVI_PEEK_PLAN) {
      ccz::sync(h);
      out_host[0] = B.nchunk; out_host[1] = B.rc; out_host[2] = B.NS;
      for (int i = 0; i < S.M; ++i) out_host[3 + i] = S.shape.ns[i];
    } else {
      ccz::fail(CCZ_EINVAL, "svi: unknown buffer %d", what);
    }
  })
}

int ccz_svi_get_result(ccz_handle h, void* state, double* loc_host, double* rho_host, double* losses_host) {
  CCZ_GUARD(h, {
    ccz::SviState& S = *ccz::as_state<ccz::SviState>("svi", state);
    const ccz::SviBuf& B = S.B;
    if (!S.has_init) ccz::fail(CCZ_EINVAL, "svi: ccz_svi_set_init has not been called");
    if (loc_host) ccz::d2h(h, loc_host, B.loc, size_t(B.N) * 8);
    if (rho_host) ccz::d2h(h, rho_host, B.rho, size_t(B.N) * 8);
    if (losses_host) ccz::d2h(h, losses_host, B.loss, size_t(B.total) * 8);
  })
}

int ccz_colsumsq_weighted(ccz_handle h, int dtype, const ccz_view* view, int64_t n_rows, const void* mean_dev, const double* weights_host,
                          double* out_host) {
  CCZ_GUARD(h, {
    if (!view || !view->data || !weights_host || !out_host || n_rows < 1 || n_rows > (int64_t(1) << 30) || view->cols < 1 ||
        view->ld < view->cols)
      ccz::fail(CCZ_EINVAL, "colsumsq_weighted: bad argument");
    ccz::check_dtype("colsumsq_weighted", dtype);
    int sc, src;
    ccz::row_chunks(n_rows, 64, &sc, &src);
    const int64_t p = view->cols;
    ccz::DBuf part(h, int64_t(sc) * p), wt(h, p), out(h, 1);
    ccz::h2d(h, wt, weights_host, size_t(p) * 8);
    ccz::by_dtype(dtype, [&](auto t) {
      using T = decltype(t);
      hipLaunchKernelGGL((ccz::k_svi_colsq<T>), dim3(unsigned((p + 255) / 256), unsigned(sc)), dim3(256), 0, ccz::stream(h),
                         static_cast<const T*>(view->data), static_cast<const T*>(mean_dev), view->ld, p, int(n_rows), src, part);
      CCZ_LAUNCH_CHECK();
    });
    hipLaunchKernelGGL(ccz::k_svi_colsq_fold, dim3(1), dim3(ccz::SVI_PT), 0, ccz::stream(h), part, sc, p, wt, out);
    CCZ_LAUNCH_CHECK();
    ccz::d2h(h, out_host, out, 8);
  })
}

}  // extern "C"
