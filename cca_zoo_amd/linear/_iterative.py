"""ALS models with deflation, run on the device: PLS_ALS, SCCA_PMD, ParkhomenkoCCA, SCCA_Span, SCCA_ADMM, SCCA_IPLS,
ElasticCCA.

Reference: ``cca_zoo/linear/_iterative.py:38-158`` (the loop and the target score), ``:166-223`` (PLS_ALS),
``:231-380`` (SCCA_PMD and its bisection), ``:631-722`` (SCCA_Span), ``:839-930`` (ParkhomenkoCCA) and
``cca_zoo/_utils/_linalg.py:76-116`` (soft threshold, deflation); ``:388-514`` (SCCA_ADMM, whose iteration is described
at the class), ``:522-623`` and ``:730-831`` (SCCA_IPLS and ElasticCCA, whose update is an elastic-net regression solved
on the device; see :class:`_BaseElasticNet`).  The first four models share one sweep: for every view,
``t = normalise(sum_{j != i} X_j w_j)``, ``raw = X_i' t``, then the model's rule turns ``raw`` into ``w_i``.  Every sweep
runs in libccz (``csrc/als.hip``); the host draws the initial vectors of all dimensions up front (they do not depend on
results), uploads them and enqueues sweeps in chunks behind a device stop word.

The views are never copied or rewritten.  After ``d`` dimensions the reference's deflated view is
``(I - Q_i Q_i') (X_i - mu_i)`` with ``Q_i`` the normalised scores, so the device reads the original rows in their own
precision and corrects the two n-vectors of an update instead (DESIGN.md "ALS models").
"""

from __future__ import annotations

import ctypes as C
import warnings
from numbers import Integral, Real
from typing import Any, ClassVar

import numpy as np
from sklearn.utils._param_validation import Interval

from cca_zoo_amd._base import BaseModel
from cca_zoo_amd._utils._resident import (MEANS_COLMEANS, ResidentViews, check_limits, fit_state, refuse_row_sharded,
                                           run_chunks)
from cca_zoo_amd._utils._validation import perview_parameter

#: sweeps per ``ccz_als_sweeps`` call: one host wait (for the chunk two calls back) per chunk
CHUNK_SWEEPS = 8
#: limits of the device path (``csrc/als.hip``)
MAX_DIMS, MAX_VIEWS = 32, 8
#: rule codes of ``ccz_als_create`` (``include/ccz.h``)
RULE_NORMALISE, RULE_SOFT_FIXED, RULE_SOFT_L1, RULE_TOP_S, RULE_ADMM, RULE_ENET = 0, 1, 2, 3, 4, 5
#: SCCA_ADMM: the largest ``min(n, p_i)`` (the side of the Gram ``csrc/als.hip`` keeps per view)
ADMM_MAX_SIDE = 16384
#: SCCA_IPLS / ElasticCCA: the widest view (``csrc/als.hip`` keeps a ``p_i x p_i`` Gram per view), the CD sweeps one solve
#: may take (scikit-learn's ``max_iter``)
ENET_MAX_P, ENET_CAP = 16384, 1000


def initial_vectors(random_state, p, k):
    """The reference's initial vectors of all ``k`` dimensions, (k, sum p): one ``default_rng(random_state)``; per
    dimension and view one ``standard_normal(p_i)``, normalised (``_iterative.py:80-89``)."""
    rng = np.random.default_rng(random_state)
    out = np.empty((k, sum(p)))
    for d in range(k):
        off = 0
        for pi in p:
            w = rng.standard_normal(pi)
            out[d, off:off + pi] = w / np.linalg.norm(w)
            off += pi
    return out


class _BaseIterative(BaseModel):
    """Alternating updates with deflation on the device (see module docstring).

    Differences from the reference, on purpose:

    - ``fit`` inside :func:`cca_zoo_amd.row_sharded` raises ``NotImplementedError``.
    - At most 32 latent dimensions and 8 views.
    - The views are never copied: the reference rewrites a float64 copy of every view once per dimension; here the
      rows are read where they lie (float32 views as float32) and device tensors are left bit-unchanged.

    As in the reference, everything after centring is float64 for float32 views too: ``weights_`` are float64,
    ``means_`` keep the input dtype.

    **Sparse views** (not in the reference, which refuses them).  PLS_ALS, SCCA_PMD, ParkhomenkoCCA and SCCA_Span take
    ``scipy.sparse`` matrices and arrays of any format, alone or next to dense host arrays (not next to CUDA tensors).  A
    sparse view is never densified and never rewritten: it is uploaded once in canonical CSR and CSC form (after scipy's
    full format check) and centring is implicit, ``(X - 1 mu') w = X w - (mu' w) 1`` and ``(X - 1 mu')' t = X' t - mu (1' t)``.
    No ``x - mu`` element is formed, so there is no float32 rounding of ``x - mu`` on this path (the difference from dense
    float32 views): stored values are widened exactly, every product and sum is float64, and float32 and float64 sparse
    views holding the same numbers give the same bits.  ``means_`` of a sparse view are float64.  The comparator of a
    sparse fit is the dense float64 fit of ``toarray()``.  ``transform``, ``score`` and the correlations take sparse views
    and return dense float64 variates; ``get_factor_loadings`` needs a view's p x p moments and raises ``ValueError`` on
    a sparse view.  SCCA_ADMM, SCCA_IPLS and ElasticCCA need the Gram of a view and raise ``ValueError``.

    ``n_iter_`` (not in the reference) lists the sweeps taken per latent dimension; ``last_delta_`` the largest weight
    change of each dimension's last sweep.
    """

    _parameter_constraints: ClassVar[dict[str, list[Any]]] = {
        **BaseModel._parameter_constraints,
        "max_iter": [Interval(Integral, 1, None, closed="left")],
        "tol": [Interval(Real, 0, None, closed="left")],
        "random_state": [Integral, None],
    }
    _rule = RULE_NORMALISE
    #: False on the models whose rule needs the Gram of a view (SCCA_ADMM, SCCA_IPLS, ElasticCCA)
    _sparse_views = True

    def __init__(
        self,
        latent_dimensions: int = 1,
        center: bool = True,
        max_iter: int = 500,
        tol: float = 1e-6,
        random_state: int | None = None,
    ) -> None:
        super().__init__(latent_dimensions=latent_dimensions, center=center)
        self.max_iter = max_iter
        self.tol = tol
        self.random_state = random_state

    def _rule_parameters(self, p) -> list[float]:
        """One number per view for the rule (``ccz_als_create``'s ``rule_param``)."""
        return [0.0] * len(p)

    def _check_shapes(self, n, p) -> None:
        """Limits of the model beyond those of the family (raises ``ValueError``)."""

    def _setup_state(self, h, state, res) -> None:
        """Model-specific calls between ``ccz_als_create`` and the first sweep."""

    def _total_units(self, k, m) -> int:
        """The most ``ccz_als_sweeps`` units a fit can need: one per sweep."""
        return k * int(self.max_iter)

    def _after_fit(self, h, state, k) -> None:
        """Model-specific read-backs once the fit has stopped."""

    def fit(self, views, y=None):
        refuse_row_sharded(f"{type(self).__name__} alternates over whole feature vectors, which this build does not shard "
                           "by rows")
        self._validate_params()
        # the means of device rows in NumPy's own order of summation (ccz_als_colmeans): torch's tree-ordered float32 mean
        # differs from v.mean(axis=0) in the last bits, and with it the whole trajectory
        res = ResidentViews(views, self.center, MEANS_COLMEANS, allow_sparse=True)
        if any(res.sparse) and not self._sparse_views:
            raise ValueError(f"{type(self).__name__} needs the Gram matrix of every view and takes no scipy.sparse views; "
                             "PLS_ALS, SCCA_PMD, ParkhomenkoCCA and SCCA_Span do")
        m, n, p = len(res.p), res.n, res.p
        k = int(self.latent_dimensions)
        check_limits(k, m, MAX_DIMS, MAX_VIEWS)
        if n < 1:
            raise ValueError("at least 1 sample is required")
        self._check_shapes(n, p)
        self.n_views_, self.n_features_in_, self.n_samples_ = m, p, n
        par = self._rule_parameters(p)
        total = self._total_units(k, m)
        chunk = max(1, min(CHUNK_SWEEPS, total))
        with res:
            h = res.handle
            with fit_state(h, "als", res.code, m, (C.c_int64 * m)(*p), n, k, int(self._rule),
                           (C.c_double * m)(*[float(x) for x in par]), float(self.tol), int(self.max_iter), chunk) as state:
                self._setup_state(h, state, res)
                for i, sv in enumerate(res.sarr):
                    if sv is not None:
                        h.check(h.lib.ccz_als_set_sparse(h.raw, state, i, C.byref(sv.view)))
                w0 = np.ascontiguousarray(initial_vectors(self.random_state, p, k))
                h.check(h.lib.ccz_als_set_init(h.raw, state, w0.ctypes.data_as(C.POINTER(C.c_double))))
                known, stopped = C.c_int64(-1), C.c_int(0)

                def sweeps(s):
                    h.check(h.lib.ccz_als_sweeps(h.raw, state, res.varr, res.marr, s, C.byref(known), C.byref(stopped)))
                    return stopped.value

                run_chunks(total, chunk, sweeps)
                dims, stop = C.c_int(0), C.c_int(0)
                iters = (C.c_int64 * k)()
                deltas = (C.c_double * k)()
                h.check(h.lib.ccz_als_status(h.raw, state, C.byref(dims), C.byref(stop), iters, deltas))
                if not stop.value or dims.value != k:
                    raise RuntimeError(f"ALS fit ended after {dims.value} of {k} dimensions")   # cannot happen: k * max_iter sweeps
                wflat = np.empty(sum(p) * k)
                h.check(h.lib.ccz_als_get_weights(h.raw, state, wflat.ctypes.data_as(C.POINTER(C.c_double))))
                self._after_fit(h, state, k)
        self.n_iter_ = [int(x) for x in iters]
        self.last_delta_ = [float(x) for x in deltas]
        weights = np.split(wflat.reshape(-1, k), np.cumsum(p)[:-1])
        self._store(weights, res.means_host(), "f32" if res.f32 else "f64", weights_like_input=False, sparse=res.sparse)
        return self

class PLS_ALS(_BaseIterative):
    r"""Alternating power iteration for PLS (multiset NIPALS), every sweep on the device.

    $w_i \leftarrow X_i^\top \bar s_{\neg i} / \|X_i^\top \bar s_{\neg i}\|_2$ with $\bar s_{\neg i}$ the normalised
    sum of the other views' scores (reference: ``cca_zoo/linear/_iterative.py:166-223``).

    Args:
        latent_dimensions: Number of latent dimensions. Default is 1.
        center: Whether to subtract column means. Default True.
        max_iter: Maximum sweeps per dimension. Default is 500.
        tol: Convergence tolerance on the largest weight change of a sweep. Default is 1e-6.
        random_state: Seed of the initial vectors.
    """


class SCCA_PMD(_BaseIterative):
    r"""Sparse CCA by penalised matrix decomposition (Witten 2009), every sweep on the device.

    Each update soft-thresholds $X_i^\top \bar s_{\neg i}$ at the level that 50 halvings of $[0, \max|raw|]$ end on
    for the L1 bound $\tau_i \sqrt{p_i}$ (reference: ``cca_zoo/linear/_iterative.py:231-380``).  As in the reference
    the bound is compared with the L1 norm of the *unnormalised* ``raw``: on data of ordinary scale ``raw`` is far
    larger than the bound and the columns come out very sparse (often one or two entries); scale the inputs down for
    denser supports.  When ``||raw||_1`` is within the bound the update is ``raw / ||raw||_2``.

    Args:
        latent_dimensions: Number of latent dimensions. Default is 1.
        center: Whether to subtract column means. Default True.
        tau: L1 bound factor(s); the bound of view ``i`` is ``tau_i * sqrt(p_i)``. Default is 1.
        max_iter: Maximum sweeps per dimension. Default is 500.
        tol: Convergence tolerance. Default is 1e-6.
        random_state: Seed of the initial vectors.
    """

    _parameter_constraints: ClassVar[dict[str, list[Any]]] = {
        **_BaseIterative._parameter_constraints,
        "tau": [Real, list],
    }
    _rule = RULE_SOFT_L1

    def __init__(
        self,
        latent_dimensions: int = 1,
        center: bool = True,
        tau: float | list[float] = 1.0,
        max_iter: int = 500,
        tol: float = 1e-6,
        random_state: int | None = None,
    ) -> None:
        super().__init__(latent_dimensions=latent_dimensions, center=center, max_iter=max_iter, tol=tol,
                         random_state=random_state)
        self.tau = tau

    def _rule_parameters(self, p):
        tau = perview_parameter("tau", self.tau, 1.0, len(p))
        return [float(t * np.sqrt(pi)) for t, pi in zip(tau, p)]


class ParkhomenkoCCA(_BaseIterative):
    r"""Sparse CCA by soft-thresholded power iteration (Parkhomenko 2009), every sweep on the device.

    $w_i \leftarrow S_{\tau_i}(X_i^\top \bar s_{\neg i})$, normalised when its norm exceeds 1e-12 (reference:
    ``cca_zoo/linear/_iterative.py:839-930``).

    Args:
        latent_dimensions: Number of latent dimensions. Default is 1.
        center: Whether to subtract column means. Default True.
        tau: Soft-threshold level(s). Default is 0.1.
        max_iter: Maximum sweeps per dimension. Default is 500.
        tol: Convergence tolerance. Default is 1e-6.
        random_state: Seed of the initial vectors.
    """

    _parameter_constraints: ClassVar[dict[str, list[Any]]] = {
        **_BaseIterative._parameter_constraints,
        "tau": [Real, list],
    }
    _rule = RULE_SOFT_FIXED

    def __init__(
        self,
        latent_dimensions: int = 1,
        center: bool = True,
        tau: float | list[float] = 0.1,
        max_iter: int = 500,
        tol: float = 1e-6,
        random_state: int | None = None,
    ) -> None:
        super().__init__(latent_dimensions=latent_dimensions, center=center, max_iter=max_iter, tol=tol,
                         random_state=random_state)
        self.tau = tau

    def _rule_parameters(self, p):
        return [float(t) for t in perview_parameter("tau", self.tau, 0.1, len(p))]


class SCCA_Span(_BaseIterative):
    r"""SpanCCA: truncated power iteration keeping the ``span`` largest entries per view, every sweep on the device.

    Entries with $|raw| \ge$ the s-th largest magnitude are kept (ties at that magnitude are all kept), then the
    vector is normalised (reference: ``cca_zoo/linear/_iterative.py:631-722``).  As in the reference the default of
    ``span`` is the width of the *first* view, for every view.

    Args:
        latent_dimensions: Number of latent dimensions. Default is 1.
        center: Whether to subtract column means. Default True.
        span: Entries to keep per view (int or list). ``None`` keeps the width of the first view; 0 keeps every entry,
            as in the reference. A negative ``span`` raises (the reference indexes the sorted magnitudes from the small
            end with it).
        max_iter: Maximum sweeps per dimension. Default is 500.
        tol: Convergence tolerance. Default is 1e-6.
        random_state: Seed of the initial vectors.
    """

    _parameter_constraints: ClassVar[dict[str, list[Any]]] = {
        **_BaseIterative._parameter_constraints,
        "span": [Integral, list, None],
    }
    _rule = RULE_TOP_S

    def __init__(
        self,
        latent_dimensions: int = 1,
        center: bool = True,
        span: int | list[int] | None = None,
        max_iter: int = 500,
        tol: float = 1e-6,
        random_state: int | None = None,
    ) -> None:
        super().__init__(latent_dimensions=latent_dimensions, center=center, max_iter=max_iter, tol=tol,
                         random_state=random_state)
        self.span = span

    def _rule_parameters(self, p):
        span = perview_parameter("span", p[0] if self.span is None else self.span, p[0], len(p))
        if any(int(s) < 0 for s in span):
            raise ValueError("span must not be negative")
        # span = 0 keeps every entry, as the reference's ``np.sort(np.abs(raw))[-0]`` (the smallest magnitude) does
        return [float(int(s)) if int(s) > 0 else float(pi) for s, pi in zip(span, p)]


class SCCA_ADMM(_BaseIterative):
    r"""Sparse CCA by ADMM (Suo et al. 2017), every iteration on the device.

    Per iteration the targets $\bar s_{\neg i}$ of all views come from the vectors the iteration started with; then,
    for each view,

    $$
    w' = w_i - \bigl(X_i^\top (X_i w_i - \bar s_{\neg i}) + \mu\,\eta_i\bigr) / L_i,\quad
    z_i = \Pi_{\|\cdot\|_2 \le 1}\, S_{\tau_i/\mu}(w' + \eta_i),\quad \eta_i \leftarrow \eta_i + w' - z_i,\quad w_i = z_i
    $$

    with $L_i = \|X_i^\top X_i\|_F / n + \mu$ on the deflated view (reference:
    ``cca_zoo/linear/_iterative.py:388-514``).  ``X_i' X_i`` is never formed: its product with ``w_i`` is two streaming
    passes over the rows, and its Frobenius norm equals that of ``X_i X_i'``, so the device keeps the float64 Gram of the
    centred view on its smaller side, ``min(n, p_i)`` squared, and deflates it with the scores of the finished
    dimensions.

    Differences from the reference, on purpose (besides those of the family):

    - ``min(n, p_i) <= 16384`` for every view (the ceiling the kernel models use for an n x n matrix); wider and taller
      views raise ``ValueError``.
    - ``mu`` must be positive (the reference divides by it).
    - float32 views: the reference multiplies ``X_i' X_i`` in float32 at the first dimension; here every product after
      centring is float64 (README "Differences").

    Args:
        latent_dimensions: Number of latent dimensions. Default is 1.
        center: Whether to subtract column means. Default True.
        tau: L1 weight(s), per view. Default is 0.1.
        mu: ADMM penalty, > 0. Default is 1.0.
        max_iter: Maximum iterations per dimension. Default is 500.
        tol: Convergence tolerance on the largest weight change of an iteration. Default is 1e-6.
        random_state: Seed of the initial vectors.
    """

    _parameter_constraints: ClassVar[dict[str, list[Any]]] = {
        **_BaseIterative._parameter_constraints,
        "tau": [Real, list],
        "mu": [Interval(Real, 0, None, closed="neither")],
    }
    _rule = RULE_ADMM
    _sparse_views = False

    def __init__(
        self,
        latent_dimensions: int = 1,
        center: bool = True,
        tau: float | list[float] = 0.1,
        mu: float = 1.0,
        max_iter: int = 500,
        tol: float = 1e-6,
        random_state: int | None = None,
    ) -> None:
        super().__init__(latent_dimensions=latent_dimensions, center=center, max_iter=max_iter, tol=tol,
                         random_state=random_state)
        self.tau = tau
        self.mu = mu

    def _rule_parameters(self, p):
        return [float(t) for t in perview_parameter("tau", self.tau, 0.1, len(p))]

    def _check_shapes(self, n, p):
        for i, pi in enumerate(p):
            if min(n, pi) > ADMM_MAX_SIDE:
                raise ValueError(f"view {i} has min(n, p) = {min(n, pi)}: SCCA_ADMM keeps a min(n, p) x min(n, p) Gram per "
                                 f"view and supports at most {ADMM_MAX_SIDE}")

    def _setup_state(self, h, state, res):
        h.check(h.lib.ccz_als_admm_setup(h.raw, state, res.varr, res.marr, float(self.mu)))


class _BaseElasticNet(_BaseIterative):
    r"""SCCA_IPLS and ElasticCCA: every view update is an elastic-net regression of a target on the deflated view,

    $$
    \hat c_i = \arg\min_c \frac{1}{2n} \|X_i c - t\|_2^2 + \alpha_i \bigl(l_1 \|c\|_1 + \tfrac{1 - l_1}{2} \|c\|_2^2\bigr),
    $$

    which the reference hands to scikit-learn's ``Lasso`` / ``ElasticNet`` with ``selection="random"`` (``Ridge`` when
    ``l1_ratio == 0``; ``cca_zoo/linear/_iterative.py:938-982``).  The contract here is the reference's *update map*, not
    its trajectory of coordinate visits: the minimiser is unique whenever ``l1_ratio < 1`` with ``alpha > 0`` or the
    deflated view has full column rank, and then it depends neither on the visiting order nor on the warm start.  The
    device solves it by blocked cyclic coordinate descent on the float64 Gram matrix of the view (``csrc/als.hip``),
    formed once per fit and deflated in place, under scikit-learn's own stop rule: after a sweep whose largest coordinate
    change is below ``tol`` times the largest coefficient, the duality gap is compared with ``tol * t't``; a solve takes at
    most 1000 sweeps.  Within a dimension a solve starts from the view's previous coefficients, the first from zero.

    ``tol`` is also the solver's tolerance, as in the reference.  The gap is formed from ``t't - c'q - c'r`` in float64,
    which cancels: a ``tol`` below about 1e-13 cannot be reached except by an accident of rounding, and such a fit runs its
    solves to the cap.

    A solve that ends on the cap without meeting the stop rule is counted, and ``fit`` then emits one ``RuntimeWarning``
    (scikit-learn's ``ConvergenceWarning`` in the reference), never silently.

    Outside the contract (nothing is claimed there beyond finite weights of the right shape and determinism):

    - ``l1_ratio = 1`` with ``p_i >= n``: the lasso objective is not strongly convex and its minimiser need not be unique;
    - any fit in which scikit-learn's own solver would not converge: the reference's result is then an unfinished random
      walk that nothing can match.

    Differences from the reference, on purpose (besides those of the family):

    - ``p_i <= 16384`` for every view (the Gram matrix is ``p_i x p_i``); wider views raise ``ValueError``.
    - ``l1_ratio = 0`` with ``alpha = 0`` and ``p_i >= n`` raises ``ValueError``: the unpenalised least-squares problem has
      no unique solution there (the reference returns whichever one its factorisation yields).
    - float32 views: in the first dimension the reference's solver runs in float32 (``ElasticNet.fit`` casts the target
      to the dtype of ``X``); here everything after centring is float64.

    ``n_inner_iter_`` (not in the reference) lists the coordinate-descent sweeps taken per latent dimension, over all
    solves.
    """

    _parameter_constraints: ClassVar[dict[str, list[Any]]] = {
        **_BaseIterative._parameter_constraints,
        "alpha": [Interval(Real, 0, None, closed="left"), list],
        "l1_ratio": [Interval(Real, 0, 1, closed="both"), list],
    }
    _rule = RULE_ENET
    _sparse_views = False
    _l1_default = 1.0
    _target_all = False
    _post_std = False

    def _penalties(self, m):
        alpha = [float(a) for a in perview_parameter("alpha", self.alpha, 0.0, m)]
        l1 = [float(x) for x in perview_parameter("l1_ratio", self.l1_ratio, self._l1_default, m)]
        if any(not (a >= 0.0 and np.isfinite(a)) for a in alpha):
            raise ValueError("alpha must be finite and not negative")
        if any(not 0.0 <= x <= 1.0 for x in l1):
            raise ValueError("l1_ratio must lie in [0, 1]")
        return alpha, l1

    def _rule_parameters(self, p):
        self._penalties(len(p))
        return [0.0] * len(p)

    def _check_shapes(self, n, p):
        alpha, l1 = self._penalties(len(p))
        for i, pi in enumerate(p):
            if pi > ENET_MAX_P:
                raise ValueError(f"view {i} has {pi} columns: {type(self).__name__} keeps a p x p Gram per view and supports at "
                                 f"most {ENET_MAX_P}")
            if l1[i] == 0.0 and alpha[i] == 0.0 and pi >= n:
                raise ValueError(f"view {i}: l1_ratio = 0 with alpha = 0 and p >= n is a least-squares problem without a unique "
                                 "solution")

    def _setup_state(self, h, state, res):
        m, n = len(res.p), res.n
        alpha, l1 = self._penalties(m)
        ridge = [1 if x == 0.0 else 0 for x in l1]
        # scikit-learn's ElasticNet scales its penalties by n; its Ridge does not
        a = [0.0 if r else n * al * x for al, x, r in zip(alpha, l1, ridge)]
        b = [al if r else n * al * (1.0 - x) for al, x, r in zip(alpha, l1, ridge)]
        h.check(h.lib.ccz_als_enet_setup(h.raw, state, res.varr, res.marr, (C.c_double * m)(*a), (C.c_double * m)(*b),
                                         (C.c_int * m)(*ridge), int(self._target_all), int(self._post_std)))

    def _total_units(self, k, m):
        # a unit advances a sweep by at least one CD sweep of one solve, or ends it
        return k * int(self.max_iter) * (m * ENET_CAP + 1)

    def _after_fit(self, h, state, k):
        inner = (C.c_int64 * k)()
        capped = C.c_int64(0)
        h.check(h.lib.ccz_als_enet_status(h.raw, state, inner, C.byref(capped)))
        self.n_inner_iter_ = [int(x) for x in inner]
        if capped.value:
            warnings.warn(f"{type(self).__name__}: {capped.value} coordinate-descent solve(s) ended on the cap of {ENET_CAP} sweeps "
                          "without reaching the duality-gap tolerance; consider a larger alpha or tol", RuntimeWarning,
                          stacklevel=3)


class SCCA_IPLS(_BaseElasticNet):
    r"""Sparse CCA by iterative penalised least squares (Mai & Zhang 2019), every solve on the device.

    For view $i$ the target is $\bar s_{\neg i}$, the normalised sum of the other views' scores; the elastic-net
    coefficients $\hat c_i$ (see :class:`_BaseElasticNet`) are divided by the population standard deviation of their score
    $X_i \hat c_i$ when that exceeds 1e-12, so that the score has unit variance (reference:
    ``cca_zoo/linear/_iterative.py:522-623``).

    Args:
        latent_dimensions: Number of latent dimensions. Default is 1.
        center: Whether to subtract column means. Default True.
        alpha: Elastic-net penalty strength(s), per view. Default is 0.
        l1_ratio: Share(s) of the L1 penalty, per view: 1 is the lasso, 0 ridge regression. Default is 1.
        max_iter: Maximum sweeps per dimension. Default is 500.
        tol: Convergence tolerance of the sweeps and of every solve. Default is 1e-6.
        random_state: Seed of the initial vectors.
    """

    _l1_default = 1.0
    _target_all = False
    _post_std = True

    def __init__(
        self,
        latent_dimensions: int = 1,
        center: bool = True,
        alpha: float | list[float] = 0.0,
        l1_ratio: float | list[float] = 1.0,
        max_iter: int = 500,
        tol: float = 1e-6,
        random_state: int | None = None,
    ) -> None:
        super().__init__(latent_dimensions=latent_dimensions, center=center, max_iter=max_iter, tol=tol,
                         random_state=random_state)
        self.alpha = alpha
        self.l1_ratio = l1_ratio


class ElasticCCA(_BaseElasticNet):
    r"""Elastic-net CCA (Waaijenborg 2008), every solve on the device.

    For every view the target is the normalised sum of ALL views' scores, view $i$'s own included, and $w_i$ is the
    elastic-net coefficient vector as it comes (see :class:`_BaseElasticNet`; reference:
    ``cca_zoo/linear/_iterative.py:730-831``).

    Args:
        latent_dimensions: Number of latent dimensions. Default is 1.
        center: Whether to subtract column means. Default True.
        alpha: Elastic-net penalty strength(s), per view. Default is 0.
        l1_ratio: Share(s) of the L1 penalty, per view. Default is 0.5.
        max_iter: Maximum sweeps per dimension. Default is 500.
        tol: Convergence tolerance of the sweeps and of every solve. Default is 1e-6.
        random_state: Seed of the initial vectors.
    """

    _l1_default = 0.5
    _target_all = True
    _post_std = False

    def __init__(
        self,
        latent_dimensions: int = 1,
        center: bool = True,
        alpha: float | list[float] = 0.0,
        l1_ratio: float | list[float] = 0.5,
        max_iter: int = 500,
        tol: float = 1e-6,
        random_state: int | None = None,
    ) -> None:
        super().__init__(latent_dimensions=latent_dimensions, center=center, max_iter=max_iter, tol=tol,
                         random_state=random_state)
        self.alpha = alpha
        self.l1_ratio = l1_ratio
