"""GFA: group factor analysis (Bayesian CCA with per-view ARD), every variational iteration on the device.

Reference: ``cca_zoo/probabilistic/_gfa.py`` (the fit, ``:184-286``; the posterior draws, ``:301-352``) and
``cca_zoo/probabilistic/_utils.py`` (``transform``, ``:11-48``; the marginal log-likelihood, ``:51-109``).  Every
coordinate-ascent iteration makes two passes over every view -- ``X_m' z`` and ``X_m w_m`` -- and ``k x k`` work besides;
both passes and the ``k x k`` algebra run in libccz (``csrc/gfa.hip``).  The host draws the initial ``z`` from
``default_rng(random_state)``, enqueues iterations in chunks behind a device stop word, and draws the posterior samples
from the same generator in the reference's order afterwards.
"""

from __future__ import annotations

import ctypes as C
from numbers import Integral, Real
from typing import Any, ClassVar

import numpy as np
from sklearn.utils._param_validation import Interval
from sklearn.utils.validation import check_is_fitted

from cca_zoo_amd._base import BaseModel
from cca_zoo_amd._utils._resident import (MEANS_COLMEANS, MEANS_TORCH, ResidentViews, check_limits, fit_state,
                                           refuse_row_sharded, run_chunks)
from cca_zoo_amd._utils._validation import validate_views
from cca_zoo_amd.probabilistic._posterior import PosteriorMeanMixin

#: iterations per ``ccz_gfa_iterations`` call: one host wait (for the chunk two calls back) per chunk; the result does
#: not depend on it
CHUNK_ITERS = 64
#: limits of the device path (``csrc/gfa.hip``)
MAX_DIMS, MAX_VIEWS = 32, 8
#: largest ``posterior_samples_["z"]`` (``num_posterior_samples x n x k`` float64) that ``fit`` draws
MAX_SAMPLE_BYTES = 2 << 30
#: CCAGFA's near-flat priors (``_gfa.py:13-16``)
_PRIOR = 1e-14


class GFA(PosteriorMeanMixin, BaseModel):
    r"""Group factor analysis: Bayesian CCA with a per-view ARD precision for every latent dimension.

    $$
    \alpha_{i,k} \sim \mathrm{Gamma}(a_0, b_0),\quad W_i[:, k] \sim \mathcal N(0, \alpha_{i,k}^{-1} I),\quad
    z \sim \mathcal N(0, I_K),\quad \tau_i \sim \mathrm{Gamma}(a_{0\tau}, b_{0\tau}),\quad
    x_i \mid z \sim \mathcal N(W_i z, \tau_i^{-1} I)
    $$

    fitted by closed-form mean-field coordinate ascent (Klami, Virtanen & Kaski 2013; the R package CCAGFA without its
    rotation step, as the reference).  ``latent_dimensions`` is an upper bound: with ``drop_k`` a dimension whose mean
    squared posterior mean falls to ``1e-7`` is pruned, and every output has ``n_components_`` columns.  The fit stops
    once the relative change of ``z`` stayed below ``tol`` for 1000 consecutive iterations without a prune, or after
    ``max_iter``.

    Fitted attributes: ``weights_`` (float64, ``p_i x n_components_``), ``means_`` (input dtype),
    ``view_relevance_`` (posterior mean of $\alpha$, ``n_views x n_components_``), ``n_iter_``, ``n_components_``,
    ``posterior_samples_`` (``z``, ``alpha``, ``W_i``, ``log_psi_i`` as in the reference), ``prune_iterations_`` (not
    in the reference: the 1-based iteration of every prune).

    ``transform`` returns a ONE-element list, the posterior mean of the shared ``z``; ``score`` and the correlations
    use each view's own projection ``(X_i - mean_i) W_i``.

    Differences from the reference, on purpose:

    - ``fit`` inside :func:`cca_zoo_amd.row_sharded` raises ``NotImplementedError``.
    - At most 32 latent dimensions and 8 views.
    - ``num_posterior_samples * n * n_components_ * 8`` bytes may not exceed 2 GiB: ``fit`` raises ``ValueError`` and
      asks for fewer samples (skipping the draw would change every later draw).
    - The views are never copied: the reference makes a float64 copy of every view; here the rows are read where they
      lie (float32 views as float32) and device tensors are left bit-unchanged.

    Args:
        latent_dimensions: Upper bound on the number of latent components. Default is 1.
        center: Whether to subtract column means. Default True.
        max_iter: Maximum number of iterations. Default is 10000.
        tol: Bound on the relative Frobenius change of ``z`` between iterations. Default is 1e-4.
        drop_k: Whether to prune latent dimensions. Default True.
        num_posterior_samples: Draws in ``posterior_samples_``. Default is 1000.
        random_state: Seed of the initial ``z`` and of the posterior draws. Default is 0.
    """

    _parameter_constraints: ClassVar[dict[str, list[Any]]] = {
        **BaseModel._parameter_constraints,
        "max_iter": [Interval(Integral, 1, None, closed="left")],
        "tol": [Interval(Real, 0, None, closed="left")],
        "drop_k": ["boolean"],
        "num_posterior_samples": [Interval(Integral, 1, None, closed="left")],
        "random_state": [Integral, None],
    }

    def __init__(
        self,
        latent_dimensions: int = 1,
        center: bool = True,
        max_iter: int = 10000,
        tol: float = 1e-4,
        drop_k: bool = True,
        num_posterior_samples: int = 1000,
        random_state: int = 0,
    ) -> None:
        super().__init__(latent_dimensions=latent_dimensions, center=center)
        self.max_iter = max_iter
        self.tol = tol
        self.drop_k = drop_k
        self.num_posterior_samples = num_posterior_samples
        self.random_state = random_state

    # -- fit -------------------------------------------------------------------------------------------------------
    def fit(self, views, y=None):
        """Fit to a list of (n_samples, n_features_i) host arrays or CUDA tensors."""
        refuse_row_sharded("GFA updates whole feature vectors and the shared latent variable in turn, which this build does not "
                           "shard by rows")
        self._validate_params()
        res = ResidentViews(views, self.center, MEANS_COLMEANS)
        m, n, p = len(res.p), res.n, res.p
        k = int(self.latent_dimensions)
        s = int(self.num_posterior_samples)
        check_limits(k, m, MAX_DIMS, MAX_VIEWS)
        if n < 2:
            raise ValueError("at least 2 samples are required")
        self._check_sample_size(s, n, k)       # before any device work: pruning can only shrink it
        self.n_views_, self.n_features_in_, self.n_samples_ = m, p, n
        total = int(self.max_iter)
        chunk = max(1, min(int(CHUNK_ITERS), total))
        rng = np.random.default_rng(self.random_state)
        z0 = np.ascontiguousarray(rng.standard_normal((n, k)))
        pd = C.POINTER(C.c_double)
        with res:
            h = res.handle
            with fit_state(h, "gfa", res.code, m, (C.c_int64 * m)(*p), n, k, float(self.tol), total, int(bool(self.drop_k)),
                           chunk) as state:
                h.check(h.lib.ccz_gfa_set_init(h.raw, state, z0.ctypes.data_as(pd)))
                h.check(h.lib.ccz_gfa_setup(h.raw, state, res.varr, res.marr))
                known, stopped = C.c_int64(-1), C.c_int(0)

                def iterations(step):
                    h.check(h.lib.ccz_gfa_iterations(h.raw, state, res.varr, res.marr, step, C.byref(known), C.byref(stopped)))
                    return stopped.value

                run_chunks(total, chunk, iterations)
                iters, stop, ka, stable, nprune = C.c_int64(0), C.c_int(0), C.c_int(0), C.c_int(0), C.c_int(0)
                rel = C.c_double(0.0)
                piters, pk = (C.c_int64 * MAX_DIMS)(), (C.c_int * MAX_DIMS)()
                h.check(h.lib.ccz_gfa_status(h.raw, state, C.byref(iters), C.byref(stop), C.byref(ka), C.byref(stable),
                                             C.byref(rel), C.byref(nprune), piters, pk))
                if not stop.value:
                    raise RuntimeError(f"GFA fit ended after {iters.value} of {total} iterations")   # cannot happen
                kk = ka.value
                z, cov_z = np.empty((n, kk)), np.empty((kk, kk))
                w, cov_w = np.empty((sum(p), kk)), np.empty((m, kk, kk))
                alpha, b_ard = np.empty((m, kk)), np.empty((m, kk))
                tau, b_tau = np.empty(m), np.empty(m)
                h.check(h.lib.ccz_gfa_get_result(h.raw, state, C.byref(ka), *[a.ctypes.data_as(pd) for a in
                                                                              (z, cov_z, w, cov_w, alpha, b_ard, tau, b_tau)]))
        if not all(np.all(np.isfinite(a)) for a in (z, cov_z, w, cov_w, alpha, tau)):
            raise np.linalg.LinAlgError("GFA: an update lost positive definiteness (the reference's Cholesky raises here)")
        self.n_iter_ = int(iters.value)
        self.n_components_ = int(kk)
        self.prune_iterations_ = [int(piters[i]) for i in range(nprune.value)]
        self.last_rel_change_ = float(rel.value)
        weights = np.split(w, np.cumsum(p)[:-1])
        self._draw_posterior_samples(rng, z, cov_z, weights, cov_w, b_ard, b_tau, n, p)
        self._store(weights, res.means_host(), "f32" if res.f32 else "f64", weights_like_input=False)
        self.view_relevance_ = alpha
        return self

    def _check_sample_size(self, s, n, k):
        if s * n * k * 8 > MAX_SAMPLE_BYTES:
            raise ValueError(
                f"num_posterior_samples={s}: posterior_samples_['z'] would hold {s} x {n} x {k} float64 values "
                f"({s * n * k * 8 / 2 ** 30:.1f} GiB, the limit is {MAX_SAMPLE_BYTES >> 30} GiB); lower num_posterior_samples"
            )

    def _draw_posterior_samples(self, rng, z, cov_z, w, cov_w, b_ard, b_tau, n, p):
        """The reference's draws in its order and shapes (``_gfa.py:326-352``): z noise, tau, alpha, then per view the
        W noise; ``log_psi_i`` is the log of ``1 / tau`` broadcast over the view's features."""
        s, m, k = int(self.num_posterior_samples), len(w), z.shape[1]
        a_ard = _PRIOR + np.array(p) / 2.0
        a_tau = _PRIOR + n * np.array(p) / 2.0
        samples = {}
        chol_z = np.linalg.cholesky(cov_z)
        samples["z"] = z[np.newaxis, :, :] + rng.standard_normal((s, *z.shape)) @ chol_z.T
        tau_samples = np.stack([rng.gamma(a_tau[i], 1.0 / b_tau[i], size=s) for i in range(m)], axis=1)
        samples["alpha"] = np.stack([rng.gamma(a_ard[i], 1.0 / b_ard[i], size=(s, k)) for i in range(m)], axis=1)
        for i in range(m):
            chol_w = np.linalg.cholesky(cov_w[i])
            samples[f"W_{i}"] = w[i][np.newaxis, :, :] + rng.standard_normal((s, p[i], k)) @ chol_w.T
            samples[f"log_psi_{i}"] = np.log(1.0 / tau_samples[:, i])[:, np.newaxis] * np.ones((1, p[i]))
        self.posterior_samples_ = samples

    # -- after the fit (transform, the correlations' variates: PosteriorMeanMixin) ---------------------------------
    def log_likelihood(self, views) -> float:
        """Mean per-sample marginal log-likelihood with ``z`` integrated out (``_utils.py:51-109``).  The noise
        variance is constant within a view, so ``x' Psi^-1 x`` needs ``sum fl(x - mean)^2`` per view (one device pass,
        ``ccz_gfa_sumsq``) and the Woodbury correction the ``n x k`` projection; no ``n x P`` array is formed."""
        check_is_fitted(self)
        validated = validate_views(views, check_finite=False)
        psi, psi_inv = self._psi_inv()
        n = int(validated[0].shape[0])
        quad_diag = 0.0
        res = ResidentViews(validated, False, MEANS_TORCH)
        with res:
            h = res.handle
            dt = np.float32 if res.f32 else np.float64
            for i in range(self.n_views_):
                if len(np.unique(psi_inv[i])) != 1:
                    raise ValueError("log_likelihood expects one noise variance per view")
                mu = h.to_device(np.asarray(self.means_[i], dtype=dt)) if self.center else None
                out = C.c_double(0.0)
                h.check(h.lib.ccz_gfa_sumsq(h.raw, res.code, C.byref(res.varr[i]), n, C.c_void_p(mu.ptr if mu else None),
                                            C.byref(out)))
                quad_diag += float(psi_inv[i][0]) * out.value
        return self._woodbury_log_likelihood(validated, psi, psi_inv, quad_diag)
