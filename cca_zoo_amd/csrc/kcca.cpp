// KCCA / KGCCA solve drivers (reference: cca_zoo/nonparametric/_kcca.py, _kgcca.py).
//
// Both models only ever touch a kernel matrix K_i through polynomials in it, so each K_i is eigendecomposed ONCE
// (K_i = U_i diag(l_i) U_i', syev_full: E_i = U_i' as rows) and everything else is diagonal scaling in that basis:
//   B_i = c_i K_i + (1 - c_i) K_i^2  has eigenvalues b_i = c_i l_i + (1 - c_i) l_i^2 (+ the shift), same vectors;
//   Kc_i B_i^-1/2 = H U_i diag(l_i / sqrt(b_i))  with H the column-centring projector (np.cov centres K's columns);
//   K_i B_i^-1 K_i = U_i diag(l_i^2 / b_i) U_i';   pinv(K_i) = U_i diag(1 / l_i, NumPy's cutoff) U_i'.
// KCCA with two views is then the top-k SVD of the whitened cross-covariance (ccz_svd_topk); more views take a
// dense EVD of the whitened (M n)-sized A.  KGCCA's Q is G G' with G = [sqrt(mu_i) U_i diag(l_i / sqrt(b_i))], so its
// top-k eigenvectors are the top-k right singular vectors of G' (formed directly).  Host work: the n eigenvalues per view and k-sized
// bookkeeping.  This file is not part of the host test double (tests/hostsim builds solve.cpp only).
//
// CCZ_TRACE_PHASES=1 times the phases of both drivers (ops.h: PhaseTimer).
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <new>
#include <numeric>
#include <string>
#include <vector>

#include "ops.h"
#include "abi_guard.h"

namespace ccz {
namespace {

void check_common(double* const* K, int m, int64_t n, int k, int min_views) {
  if (!K || m < min_views || n < 2 || k < 1) fail(CCZ_EINVAL, "bad argument");
  for (int i = 0; i < m; ++i)
    if (!K[i]) fail(CCZ_EINVAL, "null kernel matrix %d", i);
  if (k > n) fail(CCZ_EINVAL, "latent_dimensions (%d) exceeds the number of samples (%lld)", k, (long long)n);
}

// E (n x n) <- eigenvectors of K as rows, l (host, descending) <- eigenvalues; K is destroyed
void eig_kernel(ccz_ctx* c, double* K, int64_t n, double* E, std::vector<double>& l) {
  syev_full(c, K, n, l, E, n);
  for (double v : l)
    if (!std::isfinite(v)) fail(CCZ_EINVAL, "kernel matrix has non-finite entries");
}

// out (rows x cols) = diag(scale) in (ld cols)
void scale_rows(ccz_ctx* c, int64_t rows, int64_t cols, const double* in, const std::vector<double>& scale, double* out) {
  std::vector<int64_t> id(rows);
  std::iota(id.begin(), id.end(), 0);
  gather_rows(c, rows, cols, in, cols, id.data(), scale.data(), out, cols);
}

// X (rows x n) <- X - rowmean(X) 1'
void centre_rows(ccz_ctx* c, int64_t rows, int64_t n, double* X, const double* ones, double* tmp) {
  gemm(c, false, false, rows, 1, n, 1.0 / double(n), X, n, ones, 1, 0.0, tmp, 1);
  gemm(c, false, false, rows, n, 1, -1.0, tmp, 1, ones, n, 1.0, X, n);
}

// top-k singular triplets of T (p x q, row-major) through the ABI entry (solve.cpp): U (p x kk), V (q x kk) row-major
int svd_topk(ccz_ctx* c, const double* T, int64_t p, int64_t q, int k, double* U, double* s_dev, double* V) {
  const int rc = ccz_svd_topk(c, T, p, q, k, U, s_dev, V);
  if (rc != CCZ_OK) fail(rc, "%s", c->err.c_str());
  return int(std::min<int64_t>({int64_t(k), p, q}));
}

void kcca_solve_impl(ccz_ctx* c, double* const* K, int m, int64_t n, const double* cr, double eps, int k, double* W,
                     double* vals_host, int* k_out) {
  check_common(K, m, n, k, 2);
  if (!cr) fail(CCZ_EINVAL, "null argument");
  if (m > 2 && int64_t(m) * n > 16384)
    fail(CCZ_EINVAL, "KCCA with %d views solves a dense (n_views * n_samples)-sized eigenproblem: %lld > 16384", m,
         (long long)(int64_t(m) * n));
  PhaseTimer ph(c, "kcca");
  std::vector<DBuf> E;
  std::vector<std::vector<double>> l(m);
  for (int i = 0; i < m; ++i) {
    E.emplace_back(c, n * n);
    eig_kernel(c, K[i], n, E[i], l[i]);
  }
  ph.mark("eigensolve");
  // one global shift: the smallest eigenvalue of blockdiag(c_i K_i + (1 - c_i) K_i^2)
  double bmin = INFINITY;
  std::vector<std::vector<double>> b(m);
  for (int i = 0; i < m; ++i) {
    b[i].resize(n);
    for (int64_t j = 0; j < n; ++j) {
      b[i][j] = cr[i] * l[i][j] + (1.0 - cr[i]) * l[i][j] * l[i][j];
      bmin = std::min(bmin, b[i][j]);
    }
  }
  const double shift = bmin < eps ? eps - bmin : 0.0;
  // Pt_i = diag(l / sqrt(b)) E_i with centred rows = (Kc_i U_i diag(b^-1/2))'; it takes K_i's (destroyed) storage
  DBuf ones(c, n), tmp(c, n);
  fill2d(c, 1, n, ones, n, 1.0);
  std::vector<std::vector<double>> winv(m);
  for (int i = 0; i < m; ++i) {
    std::vector<double> s(n);
    winv[i].resize(n);
    for (int64_t j = 0; j < n; ++j) {
      const double bb = b[i][j] + shift;
      s[j] = l[i][j] / std::sqrt(bb);
      winv[i][j] = 1.0 / std::sqrt(bb);
    }
    scale_rows(c, n, n, E[i], s, K[i]);
    centre_rows(c, n, n, K[i], ones, tmp);
  }
  const double inv_n1 = 1.0 / double(n - 1);
  int kk;
  if (m == 2) {
    DBuf T(c, n * n), U(c, n * k), V(c, n * k), sv(c, k);
    gemm(c, false, true, n, n, n, inv_n1, K[0], n, K[1], n, 0.0, T, n);
    ph.mark("covariance");
    kk = svd_topk(c, T, n, n, k, U, sv, V);
    d2h(c, vals_host, sv, size_t(kk) * 8);
    ph.mark("topk");
    // v_1 = U_1 diag(b^-1/2) u,  v_2 likewise  (the 1/sqrt(2) of the eigenvector and the sqrt(M) of v'Bv/M = 1 cancel)
    DBuf X(c, n * kk);
    scale_rows(c, n, kk, U, winv[0], X);
    gemm(c, true, false, n, kk, n, 1.0, E[0], n, X, kk, 0.0, W, kk);
    scale_rows(c, n, kk, V, winv[1], X);
    gemm(c, true, false, n, kk, n, 1.0, E[1], n, X, kk, 0.0, W + n * kk, kk);
  } else {
    const int64_t p = int64_t(m) * n;
    DBuf T(c, p * p), Vr(c, p * p);
    fill2d(c, p, p, T, p, 0.0);
    for (int i = 0; i < m; ++i)
      for (int j = i + 1; j < m; ++j)
        gemm(c, false, true, n, n, n, inv_n1, K[i], n, K[j], n, 0.0, T.get() + i * n * p + j * n, p);
    mirror_upper(c, p, T, p);
    ph.mark("covariance");
    std::vector<double> lam;
    syev_full(c, T, p, lam, Vr, p);
    kk = k;
    for (int t = 0; t < kk; ++t) vals_host[t] = lam[t];
    ph.mark("topk");
    DBuf Y(c, n * kk), X(c, n * kk);
    const double sm = std::sqrt(double(m));
    for (int i = 0; i < m; ++i) {
      std::vector<double> sc(n);
      for (int64_t j = 0; j < n; ++j) sc[j] = sm * winv[i][j];
      transpose(c, kk, n, Vr.get() + i * n, p, Y, kk);
      scale_rows(c, n, kk, Y, sc, X);
      gemm(c, true, false, n, kk, n, 1.0, E[i], n, X, kk, 0.0, W + i * n * kk, kk);
    }
  }
  ph.mark("weights");
  sync(c);
  *k_out = kk;
}

void kgcca_solve_impl(ccz_ctx* c, double* const* K, int m, int64_t n, const double* cr, const double* mu, double eps, int k,
                      double* W, double* vals_host, int* k_out) {
  check_common(K, m, n, k, 1);
  if (!cr || !mu) fail(CCZ_EINVAL, "null argument");
  for (int i = 0; i < m; ++i)
    if (!(mu[i] >= 0.0)) fail(CCZ_EINVAL, "view_weights must be non-negative (view %d: %g)", i, mu[i]);
  PhaseTimer ph(c, "kgcca");
  std::vector<DBuf> E;
  std::vector<std::vector<double>> l(m);
  for (int i = 0; i < m; ++i) {
    E.emplace_back(c, n * n);
    eig_kernel(c, K[i], n, E[i], l[i]);
  }
  ph.mark("eigensolve");
  // Gt (M n x n): block i = diag(sqrt(mu_i) l / sqrt(b_i + shift_i)) E_i, so that Q = Gt' Gt
  const int64_t p = int64_t(m) * n;
  DBuf Gt(c, p * n);
  for (int i = 0; i < m; ++i) {
    double bmin = INFINITY;
    std::vector<double> b(n), s(n);
    for (int64_t j = 0; j < n; ++j) {
      b[j] = cr[i] * l[i][j] + (1.0 - cr[i]) * l[i][j] * l[i][j];
      bmin = std::min(bmin, b[j]);
    }
    const double shift = bmin < eps ? eps - bmin : 0.0;
    for (int64_t j = 0; j < n; ++j) s[j] = std::sqrt(mu[i]) * l[i][j] / std::sqrt(b[j] + shift);
    scale_rows(c, n, n, E[i], s, Gt.get() + i * n * n);
  }
  ph.mark("covariance");
  DBuf T(c, n * k), sv(c, k);
  // T = the top-k right singular vectors of Gt (M n x n), i.e. the left ones of G = Gt'
  const int kk = svd_topk(c, Gt, p, n, k, nullptr, sv, T);
  std::vector<double> s(kk);
  d2h(c, s.data(), sv, size_t(kk) * 8);
  for (int t = 0; t < kk; ++t) vals_host[t] = s[t] * s[t];
  ph.mark("topk");
  // weights_i = U_i diag(pinv(l_i)) U_i' T
  DBuf X(c, n * kk), X2(c, n * kk);
  for (int i = 0; i < m; ++i) {
    double lmax = 0.0;
    for (double v : l[i]) lmax = std::max(lmax, std::fabs(v));
    const double cut = 1e-15 * lmax;
    std::vector<double> pinv(n);
    for (int64_t j = 0; j < n; ++j) pinv[j] = std::fabs(l[i][j]) > cut ? 1.0 / l[i][j] : 0.0;
    gemm(c, false, false, n, kk, n, 1.0, E[i], n, T, kk, 0.0, X, kk);
    scale_rows(c, n, kk, X, pinv, X2);
    gemm(c, true, false, n, kk, n, 1.0, E[i], n, X2, kk, 0.0, W + i * n * kk, kk);
  }
  ph.mark("weights");
  sync(c);
  *k_out = kk;
}

}  // namespace
}  // namespace ccz


extern "C" {

int ccz_kcca_solve(ccz_handle h, double* const* K_dev, int n_views, int64_t n, const double* c, double eps, int k,
                   double* weights_dev, double* vals_host, int* k_out) {
  CCZ_GUARD(h, {
    if (!weights_dev || !vals_host || !k_out) ccz::fail(CCZ_EINVAL, "null argument");
    ccz::kcca_solve_impl(h, K_dev, n_views, n, c, eps, k, weights_dev, vals_host, k_out);
  })
}

int ccz_kgcca_solve(ccz_handle h, double* const* K_dev, int n_views, int64_t n, const double* c,
                    const double* view_weights, double eps, int k, double* weights_dev, double* vals_host, int* k_out) {
  CCZ_GUARD(h, {
    if (!weights_dev || !vals_host || !k_out) ccz::fail(CCZ_EINVAL, "null argument");
    ccz::kgcca_solve_impl(h, K_dev, n_views, n, c, view_weights, eps, k, weights_dev, vals_host, k_out);
  })
}

}  // extern "C"
