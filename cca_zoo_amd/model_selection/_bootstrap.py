"""bootstrap -- resampled weights and canonical correlations of two views, whole refits on the device.

The reference has no counterpart: there, as with the estimators here, the bootstrap is a Python loop of ``B`` refits on
``[X1[idx], X2[idx]]``.  A resample changes every block of the covariance and the means, so nothing can be whitened once (as
:func:`~cca_zoo_amd.model_selection.permutation_test` does).  But a resample is fully described by its multiplicity vector
``m_b`` (``m_b[s]`` = how often row ``s`` was drawn), and its second moments are weighted sums over the rows in their stored order,

    G_b = sum_s m_b[s] x_s x_s',   s_b = sum_s m_b[s] x_s,   x_s = [x1_s, x2_s],

with no gather.  Everything after that is a (p1 + p2)-sized problem per resample:

    C = (G_b - s_b s_b' / n) / (n - 1),  R_i = (1 - c_i) C_ii + c_i I = L_i L_i',  T = L_1^-1 C_12 L_2^-T = U S V',
    W_1 = L_1^-T U_k,  W_2 = L_2^-T V_k.

``tests/boot_restatement.py`` is the float64 NumPy form the device is held to.

Device side: the full-sample column means in a fixed order of summation (``ccz_als_colmeans``), ``ccz_transform`` with an identity
weight matrix for the shifted views ``X_i - 1 mu_i'`` (covariances do not change under a shift, and the shift removes the
cancellation in ``G - s s' / n``), then ``ccz_boot_rcca`` (``csrc/boot.hip``): weighted moments on the fp64 matrix pipe and, per resample, one
workgroup that factors, solves and runs a one-sided Jacobi SVD with vectors.  The host draws the indices with NumPy and counts
them (``np.bincount``), one chunk ahead of the device (``_resample.py``, shared with ``_permutation.py``); with
``draws="device"`` the multiplicities are drawn on the device instead (``ccz_draw_counts``, ``csrc/draw.hip``), straight into the
slot the moments read.  Signs and summaries are the host's: a sign flip is exact.  With ``method="BCa"`` the delete-group
jackknife (``_jackknife.py``, ``ccz_jack_rcca``) runs on the same shifted views and the intervals are bias-corrected and accelerated.
"""

from __future__ import annotations

import ctypes as C
from dataclasses import dataclass
from numbers import Integral, Real
from typing import Any

import numpy as np

from cca_zoo_amd import _backend
from cca_zoo_amd._utils._resident import acquire, release
from cca_zoo_amd.model_selection import _resample
from cca_zoo_amd.model_selection._resample import MAX_ROWS, MAX_WIDTH, ROWS_PER_SPLIT  # noqa: F401  (the limits, for callers)

#: resamples per upload and ``ccz_boot_rcca`` call (fewer when a chunk's counts would exceed ``CHUNK_COUNT_BYTES``); the
#: result does not depend on it by a bit
CHUNK_RESAMPLES = 64
CHUNK_COUNT_BYTES = 64 << 20
#: ``info`` of ``ccz_boot_rcca`` (``include/ccz.h``: CCZ_BOOT_INFO_*)
INFO_CAUSES = {
    1: "R_1 = (1 - c_1) C_11 + c_1 I has a non-positive or non-finite pivot: the resample's view 1 is rank deficient; use c > 0",
    2: "R_2 = (1 - c_2) C_22 + c_2 I has a non-positive or non-finite pivot: the resample's view 2 is rank deficient; use c > 0",
    3: "the resample holds fewer than 2 rows",
    4: "the Jacobi sweeps of the singular value decomposition did not settle",
}


@dataclass
class BootstrapResult:
    """What :func:`bootstrap` returns; ``r = min(p1, p2)``, ``k = min(latent_dimensions, r)``, ``B = n_resamples``."""

    singular_values: np.ndarray         # (r,)    observed values (the device path with all multiplicities 1), descending
    singular_values_boot: np.ndarray    # (B, r)  the same for each resample
    singular_values_se: np.ndarray      # (r,)    std over the resamples, ddof = 1
    singular_values_ci: np.ndarray      # (2, r)  percentile interval
    weights: list                       # two (p_i, k): observed weights, largest stacked entry of each column positive
    weights_boot: list                  # two (B, p_i, k): per resample, each column aligned in sign with the observed one
    weights_se: list                    # two (p_i, k)
    weights_ci: list                    # two (2, p_i, k)
    bootstrap_ratio: list               # two (p_i, k): weights / weights_se
    estimator: Any                      # the clone fitted on the full views by its ordinary fit


@dataclass
class BCaBootstrapResult(BootstrapResult):
    """What :func:`bootstrap` returns with ``method="BCa"``: ``singular_values_ci`` and ``weights_ci`` hold the BCa intervals;
    ``J = n_groups`` jackknife replicates (:func:`~cca_zoo_amd.model_selection.jackknife`)."""

    singular_values_ci_percentile: np.ndarray = None    # (2, r)  what method="percentile" returns as singular_values_ci
    weights_ci_percentile: list = None                  # two (2, p_i, k)
    singular_values_jack: np.ndarray = None             # (J, r)  replicate g: the fit without the rows s % J == g
    weights_jack: list = None                           # two (J, p_i, k), each column aligned in sign with the observed one
    singular_values_z0: np.ndarray = None               # (r,)    bias correction
    weights_z0: list = None                             # two (p_i, k)
    singular_values_acceleration: np.ndarray = None     # (r,)
    weights_acceleration: list = None                   # two (p_i, k)
    n_groups: int = None                                # J


#: how the intervals are formed: the percentile interval, or the bias-corrected and accelerated one (needs a jackknife)
METHODS = ("percentile", "BCa")


def _jackknife():
    """The jackknife's module, imported when first needed (it imports this one)."""
    from cca_zoo_amd.model_selection import _jackknife as jk

    return jk


def draw_counts(rng, n, count):
    """``count`` x ``n`` multiplicities (int32): row ``b`` counts the ``b``-th ``rng.integers(0, n, size=n)``."""
    out = np.empty((count, n), dtype=np.int32)
    for b in range(count):
        out[b] = np.bincount(rng.integers(0, n, size=n), minlength=n)
    return out


def count_chunks(rng, n, total, chunk):
    """The ``total`` resamples of :func:`draw_counts` in chunks of at most ``chunk``, drawn as they are asked for."""
    return _resample.chunks(draw_counts, rng, n, total, chunk)


def chunk_length(n):
    """Resamples per upload: ``CHUNK_RESAMPLES``, fewer when their counts would exceed ``CHUNK_COUNT_BYTES``."""
    return _resample.chunk_length(n, CHUNK_RESAMPLES, CHUNK_COUNT_BYTES)


def orient_observed(W):
    """Flip each column of the stacked weights ``W`` ((p1 + p2) x k) so that its entry of largest magnitude (ties: the first) is
    positive; the two views of a column flip together."""
    W = np.array(W, dtype=np.float64)
    if W.size:
        lead = W[np.argmax(np.abs(W), axis=0), np.arange(W.shape[1])]
        W[:, lead < 0] *= -1.0
    return W


def orient_to(Wb, W):
    """Flip each column of every resample of ``Wb`` (B x (p1 + p2) x k) whose dot product with the observed column is < 0."""
    Wb = np.array(Wb, dtype=np.float64)
    Wb *= np.where(np.einsum("bij,ij->bj", Wb, W) < 0, -1.0, 1.0)[:, None, :]
    return Wb


def summaries(boot, confidence_level):
    """``(se, ci)``: ``std(axis=0, ddof=1)`` and the percentile interval ``quantile([(1 - cl) / 2, (1 + cl) / 2], axis=0)``."""
    boot = np.asarray(boot, dtype=np.float64)
    q = [(1.0 - confidence_level) / 2.0, (1.0 + confidence_level) / 2.0]
    return np.std(boot, axis=0, ddof=1), np.quantile(boot, q, axis=0)


def check_method(method, jackknife_groups):
    """``ValueError`` for an unknown ``method``, or ``jackknife_groups`` without the jackknife."""
    if not (isinstance(method, str) and method in METHODS):
        raise ValueError(f"bootstrap: method must be one of {list(METHODS)}, got {method!r}")
    if method == "percentile" and jackknife_groups is not None:
        raise ValueError("bootstrap: jackknife_groups needs method='BCa'; the percentile interval runs no jackknife")


def check_limits(n, p, n_resamples, confidence_level):
    """``ValueError`` for what the device path excludes, before the device is touched."""
    if isinstance(n_resamples, bool) or not isinstance(n_resamples, Integral) or n_resamples < 2:
        raise ValueError(f"n_resamples must be an integer >= 2 (a standard error needs two), got {n_resamples!r}")
    if isinstance(confidence_level, bool) or not isinstance(confidence_level, Real) or not 0.0 < confidence_level < 1.0:
        raise ValueError(f"confidence_level must be a number in (0, 1), got {confidence_level!r}")
    _resample.check_shape("bootstrap", n, p)


def _shifted(h, xptr, n, d, center):
    """The device float64 view minus its full-sample column means (``center``) as a device buffer, or ``None`` for the view as
    it is; raises for non-finite input."""
    vp = C.c_void_p
    view = _backend.View()
    view.data, view.cols, view.ld = int(xptr), d, d
    mu_d = h.alloc(d * 8)
    # the rows added in order, one thread per column: the same bits on every call (the K1 pass, ``ccz_moments``, folds its row
    # chunks with atomics, and a mean that moves in its last bit moves every bit after it)
    h.check(h.lib.ccz_als_colmeans(h.raw, _backend.F64, C.byref(view), n, vp(mu_d.ptr)))
    if not np.all(np.isfinite(h.to_host(mu_d, (d,)))):      # a NaN or an infinity anywhere in a column shows in its mean
        raise ValueError("Input contains NaN or infinity.")
    if not center:
        return None
    w_d, z_d = h.to_device(np.eye(d)), h.alloc(n * d * 8)
    # (x - mu) I: the other products of a row are exact zeros, so z is the correctly rounded x - mu in any order of summation
    h.check(h.lib.ccz_transform(h.raw, _backend.F64, vp(xptr), n, d, d, vp(mu_d.ptr), vp(w_d.ptr), d, vp(z_d.ptr), d))
    return z_d


def boot_rcca(h, n, p1, p2, x1_ptr, x2_ptr, counts_ptr, nboot, c1, c2, center, k, sv_ptr, w_ptr, info_ptr):
    """One ``ccz_boot_rcca`` call (enqueue-only); ``counts_ptr`` None = all multiplicities 1."""
    vp = C.c_void_p
    h.check(h.lib.ccz_boot_rcca(h.raw, int(n), int(p1), int(p2), vp(int(x1_ptr)), vp(int(x2_ptr)),
                                vp(int(counts_ptr)) if counts_ptr else None, int(nboot), float(c1), float(c2), int(bool(center)),
                                int(k), vp(int(sv_ptr)), vp(int(w_ptr)), vp(int(info_ptr))))


def raise_for_info(info):
    """``np.linalg.LinAlgError`` for the first non-zero ``info`` (``info[0]``: the observed sample, ``info[1 + b]``: resample b)."""
    for i in np.flatnonzero(info):
        which = "the observed sample" if i == 0 else f"resample {i - 1}"
        code = int(info[i])
        raise np.linalg.LinAlgError(f"bootstrap: {which}: {INFO_CAUSES.get(code, f'info = {code}')}")


def bootstrap(estimator, views, n_resamples=1000, confidence_level=0.95, random_state=None, *, draws="numpy", method="percentile",
              jackknife_groups=None):
    r"""Non-parametric bootstrap of the weights and singular values of a two-view CCA, rCCA or PLS.

    The rows are drawn with replacement ``n_resamples`` times (n out of n); every resample is refitted on the device from
    its multiplicity-weighted moments, without gathering rows (see the module docstring).  The observed values come from
    the same device path with all multiplicities 1.

    Args:
        estimator: an unfitted :class:`~cca_zoo_amd.linear.CCA`, :class:`~cca_zoo_amd.linear.rCCA` or
            :class:`~cca_zoo_amd.linear.PLS` (or a subclass of ``rCCA``); its ridge ``c``, ``center`` and
            ``latent_dimensions`` define the problem, ``k = min(latent_dimensions, p1, p2)`` weight columns are kept.  The
            object itself is not changed (a clone is fitted).
        views: two (n, p_i) host ``float32`` / ``float64`` arrays, or two 2-D CUDA tensors of those dtypes.  float32 views
            are widened to float64 once; everything after that is float64.
        n_resamples: ``B >= 2``.
        confidence_level: level of the percentile intervals, in (0, 1).
        random_state: seed of ``np.random.default_rng``; resample ``b`` is the ``b``-th ``rng.integers(0, n, size=n)``.
        draws: ``"numpy"`` (default): the resamples are drawn and counted on the host as above and uploaded.  ``"device"``:
            they are drawn on the device and no count array is built or uploaded by the host -- draw ``j`` of resample ``b`` picks
            row ``(splitmix64(stream(seed, b) ^ splitmix64(j)) * n) >> 64`` (``include/ccz.h``: ``ccz_draw_counts``) with
            ``seed = np.random.default_rng(random_state).integers(0, 2**64, dtype=np.uint64)``.  The two settings give
            different, equally valid random resamples: the observed values are the same bits, standard errors and intervals
            differ by Monte Carlo error only.  Either setting is reproducible from ``random_state``.
        method: ``"percentile"`` (default): the percentile interval; no jackknife runs.  ``"BCa"``: the bias-corrected and
            accelerated interval (Efron 1987, the default of ``scipy.stats.bootstrap``; the rule is that of
            :func:`~cca_zoo_amd.model_selection.bca_intervals`), which corrects the percentile interval's known first-order
            bias -- sample canonical correlations are biased upward, weights near a sign flip are skewed.  It runs the
            delete-group jackknife of :func:`~cca_zoo_amd.model_selection.jackknife` on the same device views.
        jackknife_groups: the jackknife's ``n_groups`` (``None``: ``min(n, 4096)``); only with ``method="BCa"``.

    Returns:
        :class:`BootstrapResult`.  ``se = std(axis=0, ddof=1)``, ``ci = quantile(boot, [(1 - cl) / 2, (1 + cl) / 2], axis=0)``,
        ``bootstrap_ratio = weights / weights_se``.  Each observed weight column is signed so that the entry of largest
        magnitude of the stacked column ``[w1; w2]`` is positive; each resampled column so that its stacked dot product with
        the observed column is >= 0 (the two views of a column always flip together).  With ``method="BCa"``:
        :class:`BCaBootstrapResult`, a subclass whose ``singular_values_ci`` and ``weights_ci`` are the BCa intervals; it keeps
        the percentile intervals (``*_ci_percentile``) and adds the jackknife values (``*_jack``), the bias corrections
        (``*_z0``), the accelerations (``*_acceleration``) and ``n_groups``.  An entry whose observed value lies outside its
        bootstrap values, or whose jackknife values are all equal, has a NaN interval (one ``RuntimeWarning``).

    Limits of this first cut (``ValueError`` before the device is touched): ``max(p1, p2) <= 64`` -- wider views are reduced
    first (e.g. to their leading principal components); ``n < 2^31``; ``n >= 2``; ``draws`` is one of the two names.  Sparse views and half-precision views raise
    ``TypeError``; a call inside :func:`cca_zoo_amd.row_sharded` raises ``NotImplementedError``.  A resample whose regularised
    covariance cannot be factored (with ``c = 0``: fewer distinct rows than columns) raises ``np.linalg.LinAlgError`` that
    names the resample and the remedy ``c > 0``.
    """
    def check(n, p):
        check_method(method, jackknife_groups)
        if method == "BCa":
            _jackknife().check_groups_type("jackknife_groups", jackknife_groups)
        check_limits(n, p, n_resamples, confidence_level)
        if method == "BCa":
            _jackknife().resolve_groups("jackknife_groups", n, jackknife_groups)

    est, views_, n, p, c_, center, on_device = _resample.prepare("bootstrap", "refits on all rows of one device", estimator, views, check, draws)
    B, r = int(n_resamples), min(p)
    k, pt = min(int(est.latent_dimensions), r), p[0] + p[1]

    h = _backend.handle_for(views_)
    x64, xptr = _resample.stage_f64(h, views_, on_device)  # for the column means and the shift
    sp = acquire(h, views_)
    try:
        Z = [_shifted(h, xptr[i], n, p[i], center) for i in range(2)]
        zptr = [int(z.ptr) if z is not None else xptr[i] for i, z in enumerate(Z)]
        sv, W, info = h.alloc((B + 1) * r * 8), h.alloc((B + 1) * pt * k * 8), h.alloc((B + 1) * 4)
        boot_rcca(h, n, p[0], p[1], zptr[0], zptr[1], None, 1, c_[0], c_[1], center, k, sv.ptr, W.ptr, info.ptr)
        chunk = chunk_length(n)
        if draws == "device":
            source = _resample.device_chunks(h, "counts", n, _resample.device_seed(random_state), B, chunk)
        else:
            source = count_chunks(np.random.default_rng(random_state), n, B, chunk)
        slots = _resample.run_chunks(
            h, source, min(chunk, B) * n * 4,
            lambda ptr, count, done: boot_rcca(h, n, p[0], p[1], zptr[0], zptr[1], ptr, count, c_[0], c_[1], center, k, sv.ptr + (1 + done) * r * 8,
                                               W.ptr + (1 + done) * pt * k * 8, info.ptr + (1 + done) * 4))
        sv_h, W_h = h.to_host(sv, (B + 1, r)), h.to_host(W, (B + 1, pt, k))
        info_h = h.to_host(info, (B + 1,), dtype=np.int32)
        if method == "BCa":                                # on the same shifted views, before they are released
            J = _jackknife().resolve_groups("jackknife_groups", n, jackknife_groups)
            sv_j, W_j, info_j = _jackknife().run_replicates(h, n, p, zptr, c_, center, k, J)
    finally:
        release(h, sp)
    del x64, Z, slots
    raise_for_info(info_h)
    if not np.all(np.isfinite(sv_h)) or not np.all(np.isfinite(W_h)):
        raise np.linalg.LinAlgError("bootstrap: the resampled solutions are not finite")
    W_obs = orient_observed(W_h[0])
    W_boot = orient_to(W_h[1:], W_obs)
    sv_se, sv_ci = summaries(sv_h[1:], confidence_level)
    w_se, w_ci = summaries(W_boot, confidence_level)
    cut = [slice(0, p[0]), slice(p[0], pt)]
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = W_obs / w_se
    fields = dict(singular_values=sv_h[0].copy(), singular_values_boot=sv_h[1:].copy(), singular_values_se=sv_se,
                  singular_values_ci=sv_ci, weights=[W_obs[s].copy() for s in cut],
                  weights_boot=[np.ascontiguousarray(W_boot[:, s]) for s in cut], weights_se=[w_se[s].copy() for s in cut],
                  weights_ci=[np.ascontiguousarray(w_ci[:, s]) for s in cut], bootstrap_ratio=[ratio[s].copy() for s in cut])
    if method == "percentile":
        est.fit(list(views))
        return BootstrapResult(**fields, estimator=est)
    _jackknife().raise_for_info(info_j, "bootstrap: jackknife")
    if not np.all(np.isfinite(sv_j)) or not np.all(np.isfinite(W_j)):
        raise np.linalg.LinAlgError("bootstrap: the jackknife replicates' solutions are not finite")
    W_jack = orient_to(W_j, W_obs)
    sv_bca, sv_z0, sv_a = _jackknife().bca_intervals(fields["singular_values"], fields["singular_values_boot"], sv_j, confidence_level)
    w_bca, w_z0, w_a = _jackknife().bca_intervals(W_obs, W_boot, W_jack, confidence_level)
    fields.update(singular_values_ci=sv_bca, weights_ci=[np.ascontiguousarray(w_bca[:, s]) for s in cut])
    est.fit(list(views))
    return BCaBootstrapResult(**fields, estimator=est, singular_values_ci_percentile=sv_ci,
                              weights_ci_percentile=[np.ascontiguousarray(w_ci[:, s]) for s in cut], singular_values_jack=sv_j,
                              weights_jack=[np.ascontiguousarray(W_jack[:, s]) for s in cut], singular_values_z0=sv_z0,
                              weights_z0=[w_z0[s].copy() for s in cut], singular_values_acceleration=sv_a,
                              weights_acceleration=[w_a[s].copy() for s in cut], n_groups=J)
