"""Grid search with cross-validation that reuses second moments.

Interface of ``cca_zoo/model_selection/_search.py:146-306`` (constructor, ``fit(views)``,
``cv_results_`` / ``best_*_`` attributes, ``transform`` / ``score``).  The reference hands the
stacked views to ``sklearn.model_selection.GridSearchCV``, i.e. one full ``fit`` from the data per
(setting, fold) plus one per refit: ``n_settings x n_folds + 1`` passes of O(n d^2) each.

For the moment-based estimators of this package none of that needs the data more than once:

* second moments are additive over rows, so ONE pass (K1 per test fold) gives the moments of every
  fold, their sum gives the full-data moments, and ``M_train = M_all - M_fold`` (``ccz_moments_axpby``);
* every hyper-parameter of rCCA / CCA / PLS / MCCA / GCCA (``c``, ``latent_dimensions``, ``eps``,
  ``view_weights``, ``center``) acts after K1, so a setting costs one solve (``_fit_from_moments``);
* the default score (mean over latent dimensions of the average pairwise Pearson correlation of the
  transformed held-out views, ``_search.py:70-83``) is a function of the held-out fold's moments and
  the weights: ``cov(z_i, z_j) = w_i'(G_ij - s_i s_j'/n) w_j / (n-1)`` -- two small GEMMs.

Anything else (custom ``scoring``, ``fit_params``, foreign estimators, splitters whose test sets do not
partition the rows) takes the generic route through scikit-learn, one fit per (setting, fold).
"""

from __future__ import annotations

import time
import warnings
from typing import Any

import numpy as np
from sklearn.base import BaseEstimator, clone
from sklearn.model_selection import ParameterGrid, check_cv

from cca_zoo_amd import _backend, _dist
from cca_zoo_amd._moments import compute_moments
from cca_zoo_amd._utils._validation import is_device_tensor, validate_views


class _StackedViews(BaseEstimator):
    """Generic route: presents a multiview estimator to scikit-learn as an ``(X, y)`` estimator on the
    column-stacked views (``widths`` says where to cut)."""

    def __init__(self, estimator=None, widths=()):
        self.estimator = estimator
        self.widths = widths

    def _cut(self, X):
        edges = np.cumsum([0, *self.widths])
        return [X[:, a:b] for a, b in zip(edges[:-1], edges[1:])]

    def fit(self, X, y=None, **fit_params):
        self.estimator_ = clone(self.estimator).fit(self._cut(X), **fit_params)
        return self

    def score(self, X, y=None):
        return float(np.mean(self.estimator_.score(self._cut(X))))


def _gram_reusable(estimator) -> bool:
    from cca_zoo_amd.linear import CCA, GCCA, MCCA, PLS, rCCA

    own_fits = {rCCA.fit, CCA.fit, PLS.fit, MCCA.fit, GCCA.fit}
    return isinstance(estimator, (rCCA, MCCA, GCCA)) and type(estimator).fit in own_fits


def _rows(view, idx):
    """Rows ``idx`` of a view: a zero-copy slice when they are consecutive, else a gathered copy."""
    if len(idx) and int(idx[-1]) - int(idx[0]) + 1 == len(idx) and np.all(np.diff(idx) == 1):
        return view[int(idx[0]): int(idx[-1]) + 1]
    if is_device_tensor(view):
        import torch

        return view[torch.as_tensor(idx, device=view.device)]
    return view[idx]


def score_from_moments(h, mom_sym_ptr, colsum, n_rows, dims, weights) -> float:
    """Default score of a fitted model on a row set known only through its (symmetrised) moments."""
    D, m = int(sum(dims)), len(dims)
    k = int(weights[0].shape[1])
    Wbig = np.zeros((D, m * k))
    o = 0
    for i, (d, w) in enumerate(zip(dims, weights)):
        Wbig[o:o + d, i * k:(i + 1) * k] = w
        o += d
    Wd = h.to_device(Wbig)
    Zd = h.alloc(D * m * k * 8)
    Qd = h.alloc(m * k * m * k * 8)
    h.gemm(0, 0, D, m * k, D, 1.0, mom_sym_ptr, D, Wd.ptr, m * k, 0.0, Zd.ptr, m * k)          # Z = G W
    h.gemm(1, 0, m * k, m * k, D, 1.0, Wd.ptr, m * k, Zd.ptr, m * k, 0.0, Qd.ptr, m * k)        # Q = W' G W
    Q = h.to_host(Qd, (m * k, m * k))
    sw = (colsum[:, None] * Wbig).sum(axis=0)   # no BLAS call here: see the note on host threads in DESIGN.md
    S = Q - np.outer(sw, sw) / n_rows                     # (n-1) cov of the stacked variates
    nrm = np.sqrt(np.maximum(np.diag(S), 0.0))
    nrm = np.where(nrm > 1e-12, nrm, 1.0)                 # same guard as BaseModel.pairwise_correlations
    R = S / np.outer(nrm, nrm)
    per_dim = np.zeros(k)
    for i in range(m):
        for j in range(m):
            if i != j:
                per_dim += np.diag(R[i * k:(i + 1) * k, j * k:(j + 1) * k])
    return float(np.mean(per_dim / (m * (m - 1))))


class GridSearchCV:
    """Exhaustive search over ``param_grid`` with cross-validation for multiview estimators.

    Args:
        estimator: a multiview estimator (``fit(views)`` / ``score(views)``).
        param_grid: dict (or list of dicts) of parameter name -> list of values.
        cv: number of folds or a scikit-learn splitter (default 5-fold, unshuffled).
        scoring: ``None`` = the estimator's own ``score`` averaged over latent dimensions.
        n_jobs, verbose: forwarded on the generic route (the moment route is sequential on one GPU).
        refit: fit ``best_estimator_`` on all rows with the best setting.
    """

    def __init__(self, estimator, param_grid, cv: int | Any = 5, scoring: str | None = None,
                 n_jobs: int | None = None, refit: bool = True, verbose: int = 0) -> None:
        self.estimator = estimator
        self.param_grid = param_grid
        self.cv = cv
        self.scoring = scoring
        self.n_jobs = n_jobs
        self.refit = refit
        self.verbose = verbose

    # -- public API --------------------------------------------------------------------------
    def fit(self, views, y=None, **fit_params):
        if self.scoring is None and not fit_params and _gram_reusable(self.estimator):
            validated = validate_views(views, check_finite=False, allow_bf16=True)     # (the closed-form family: bfloat16 views pass)
            n = int(validated[0].shape[0])
            splits = list(check_cv(self.cv).split(np.zeros((n, 1))))
            seen = np.zeros(n, dtype=np.int64)
            partition = True
            for train, test in splits:
                seen[test] += 1
                partition = partition and len(train) + len(test) == n and len(np.intersect1d(train, test)) == 0
            if partition and np.all(seen == 1):
                return self._fit_from_shared_moments(validated, splits)
        return self._fit_generic(views, y, **fit_params)

    def transform(self, views):
        if not self.refit:
            raise AttributeError("`transform` is not available when `refit=False`; no `best_estimator_` was "
                                 "fitted. Set `refit=True` to use it.")
        return self.best_estimator_.transform(views)

    def score(self, views, y=None) -> float:
        if not self.refit:
            raise AttributeError("`score` is not available when `refit=False`; no `best_estimator_` was fitted.")
        return float(np.mean(self.best_estimator_.score(views)))

    # -- one pass over the data ------------------------------------------------------------------
    def _fit_from_shared_moments(self, views, splits):
        """Inside ``row_sharded()`` the views are this rank's rows: the folds are cut within every shard (global fold f
        = union of the ranks' folds f), ``compute_moments`` all-reduces each fold's moments, and every rank then runs
        the same solves on the same global moments (replicated, like a sharded ``fit``)."""
        h = _backend.handle_for(views)
        candidates = list(ParameterGrid(self.param_grid))
        n_folds = len(splits)
        t_pass = time.perf_counter()
        folds = []           # (moments ptr, keepalive, rows, column sums)
        dims = kind = None
        for _, test in splits:
            mom, keep, n_f, dims, kind = compute_moments([_rows(v, test) for v in views], h)
            folds.append((mom, keep, n_f))
        D = int(sum(dims))
        n = int(sum(n_f for _, _, n_f in folds))                 # global row count (all-reduced under sharding)
        total = h.alloc((D * D + D) * 8)
        h.memset0(total.ptr, (D * D + D) * 8)
        for mom, _, _ in folds:
            h.moments_axpby(D, 1.0, mom, 1.0, total.ptr)
        h.sync()
        self.moments_pass_time_ = time.perf_counter() - t_pass

        # (setting, fold) work items: replicated moments, so inside row_sharded() every rank takes a share of the
        # solves and the score tables are summed over the ranks afterwards
        rank, world = _dist.rank_and_world(_dist.active_group())
        scores = np.zeros((len(candidates), n_folds))
        failed = np.zeros_like(scores)
        fit_t = np.zeros_like(scores)
        score_t = np.zeros_like(scores)
        train = h.alloc((D * D + D) * 8)
        for f, (mom, _, n_f) in enumerate(folds):
            mine = [ci for ci in range(len(candidates)) if (f * len(candidates) + ci) % world == rank]
            if not mine:
                continue
            h.memset0(train.ptr, (D * D + D) * 8)
            h.moments_axpby(D, 1.0, total.ptr, 1.0, train.ptr)
            h.moments_axpby(D, -1.0, mom, 1.0, train.ptr)                 # moments of the rows outside fold f
            colsum = h.to_host(mom, (D,), offset_bytes=D * D * 8)
            h.moments_symmetrize(mom, D)                                  # scoring GEMMs read full rows of G
            for ci in mine:
                params = candidates[ci]
                est = clone(self.estimator).set_params(**params)
                t0 = time.perf_counter()
                try:
                    est._fit_from_moments(h, train.ptr, n - n_f, dims, kind)
                    t1 = time.perf_counter()
                    scores[ci, f] = score_from_moments(h, mom, colsum, n_f, dims, est.weights_)
                    t2 = time.perf_counter()
                except (ValueError, np.linalg.LinAlgError, RuntimeError) as err:     # sklearn's error_score=nan
                    t1 = t2 = time.perf_counter()
                    failed[ci, f] = 1.0
                    warnings.warn(f"fit failed for {params} on fold {f}: {err}; score set to nan", RuntimeWarning)
                fit_t[ci, f], score_t[ci, f] = t1 - t0, t2 - t1
                if self.verbose:
                    print(f"[fold {f + 1}/{n_folds}] {params} score={scores[ci, f]:.6f} fit={t1 - t0:.3f}s")
        if world > 1:
            dev = getattr(h, "torch_device", None) or f"cuda:{h.device}"
            packed = _dist.allreduce_small(np.stack([scores, failed, fit_t, score_t]), dev, _dist.active_group())
            scores, failed, fit_t, score_t = packed
        scores = np.where(failed > 0, np.nan, scores)
        if np.all(np.isnan(scores)):
            raise ValueError(f"All the {scores.size} fits failed. It is very likely that your model is misconfigured "
                             "(see the warnings above for the individual failures).")
        self._finish(candidates, scores, fit_t, score_t)
        if self.refit:
            t0 = time.perf_counter()
            self.best_estimator_ = clone(self.estimator).set_params(**self.best_params_)
            self.best_estimator_._fit_from_moments(h, total.ptr, n, dims, kind)
            self.refit_time_ = time.perf_counter() - t0
        self.route_ = "shared-moments"
        del folds
        return self

    def _finish(self, candidates, scores, fit_t, score_t):
        """``cv_results_`` and the ``best_*`` attributes with scikit-learn's keys and tie rules."""
        n_folds = scores.shape[1]
        res: dict[str, Any] = {
            "mean_fit_time": fit_t.mean(axis=1), "std_fit_time": fit_t.std(axis=1),
            "mean_score_time": score_t.mean(axis=1), "std_score_time": score_t.std(axis=1),
        }
        names = sorted({k for c in candidates for k in c})
        for name in names:
            col = np.ma.MaskedArray(np.empty(len(candidates), dtype=object), mask=True)
            for i, c in enumerate(candidates):
                if name in c:
                    col[i] = c[name]
            res[f"param_{name}"] = col
        res["params"] = candidates
        for f in range(n_folds):
            res[f"split{f}_test_score"] = scores[:, f]
        mean = scores.mean(axis=1)
        res["mean_test_score"] = mean
        res["std_test_score"] = scores.std(axis=1)
        order = np.where(np.isnan(mean), -np.inf, mean)                      # failed settings rank last
        res["rank_test_score"] = (np.array([np.sum(order > v) for v in order]) + 1).astype(np.int32)   # rankdata(-x, "min")
        self.cv_results_ = res
        self.best_index_ = int(np.argmin(res["rank_test_score"]))
        self.best_score_ = float(mean[self.best_index_])
        self.best_params_ = dict(candidates[self.best_index_])
        self.n_splits_ = n_folds

    # -- generic route ---------------------------------------------------------------------------
    def _fit_generic(self, views, y=None, **fit_params):
        import sklearn.model_selection as skms

        if _dist.is_sharded():
            # scikit-learn would fit and score this rank's shard only: every rank a different, non-global cv_results_
            raise NotImplementedError(
                "GridSearchCV inside row_sharded() needs the shared-moments route (default scoring, no fit_params, an "
                "rCCA/CCA/PLS/MCCA/GCCA estimator and a splitter whose test sets partition the rows); this "
                "configuration would search each rank's local shard separately")

        arrays = [v.detach().cpu().numpy() if type(v).__module__.startswith("torch") else np.asarray(v) for v in views]
        widths = tuple(int(a.shape[1]) for a in arrays)
        grids = self.param_grid if isinstance(self.param_grid, list) else [self.param_grid]
        grids = [{f"estimator__{k}": v for k, v in g.items()} for g in grids]
        inner = skms.GridSearchCV(_StackedViews(self.estimator, widths), grids, cv=self.cv, scoring=self.scoring,
                                  n_jobs=self.n_jobs, refit=self.refit, verbose=self.verbose)
        inner.fit(np.hstack(arrays), y, **fit_params)
        self.cv_results_ = inner.cv_results_
        self.best_index_ = int(inner.best_index_)
        self.best_score_ = float(inner.best_score_)
        self.best_params_ = {k[len("estimator__"):]: v for k, v in inner.best_params_.items()}
        self.n_splits_ = inner.n_splits_
        if self.refit:
            self.best_estimator_ = inner.best_estimator_.estimator_
            self.refit_time_ = inner.refit_time_
        self.route_ = "generic"
        return self
