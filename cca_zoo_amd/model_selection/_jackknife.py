"""jackknife -- delete-group refits of a two-view CCA, rCCA or PLS on the device, and the BCa interval built on them.

Replicate ``g`` of ``J = n_groups`` is the fit on all rows except those with ``s % J == g``.  The groups are interleaved so
that row order (rows sorted by class, say) does not put a whole stratum into one group; their sizes differ by at most 1.
A replicate's moments are the full-sample moments minus those of the few rows left out,

    G_(g) = G - sum_{s in g} x_s x_s',   s_(g) = s - sum_{s in g} x_s,   N_(g) = n - |g|,

so the whole jackknife is one pass over the data for ``G`` and ``s``, one more for all the downdates together, and the
bootstrap's per-resample solve (``ccz_jack_rcca``, ``csrc/boot.hip``) -- no ``n x n`` count matrix and no ``O(n^2 p)`` work, which is what
running it as ``ccz_boot_rcca`` on 0/1 counts would cost.  ``tests/jack_restatement.py`` is the float64 NumPy form the device is
held to: one literal refit per group.

:func:`bca_intervals` is the bias-corrected and accelerated bootstrap interval (Efron 1987) by the rule of
``scipy.stats.bootstrap``; :func:`~cca_zoo_amd.model_selection.bootstrap` uses it with ``method="BCa"``.
"""

from __future__ import annotations

import ctypes as C
import warnings
from dataclasses import dataclass
from numbers import Integral
from typing import Any

import numpy as np

from cca_zoo_amd import _backend
from cca_zoo_amd._utils._resident import acquire, release
from cca_zoo_amd.model_selection import _bootstrap, _resample

#: ``n_groups=None`` means ``min(n, DEFAULT_GROUPS)``: a documented default, not a measured optimum
DEFAULT_GROUPS = 4096


@dataclass
class JackknifeResult:
    """What :func:`jackknife` returns; ``r = min(p1, p2)``, ``k = min(latent_dimensions, r)``, ``J = n_groups``."""

    singular_values: np.ndarray         # (r,)    observed values (the device path with all multiplicities 1), descending
    weights: list                       # two (p_i, k): observed weights, largest stacked entry of each column positive
    singular_values_jack: np.ndarray    # (J, r)  replicate g: the fit without the rows s % J == g
    weights_jack: list                  # two (J, p_i, k): per replicate, each column aligned in sign with the observed one
    singular_values_se: np.ndarray      # (r,)    sqrt((J - 1) / J * sum_g (theta_g - mean)^2)
    weights_se: list                    # two (p_i, k)
    singular_values_bias: np.ndarray    # (r,)    (J - 1) (mean - observed)
    weights_bias: list                  # two (p_i, k)
    n_groups: int                       # J
    estimator: Any                      # the clone fitted on the full views by its ordinary fit


def check_groups_type(name, n_groups):
    """``ValueError`` for an ``n_groups`` that is neither ``None`` nor an integer >= 2 (needs no ``n``)."""
    if n_groups is None:
        return
    if isinstance(n_groups, bool) or not isinstance(n_groups, Integral) or n_groups < 2:
        raise ValueError(f"{name} must be None or an integer >= 2, got {n_groups!r}")


def resolve_groups(name, n, n_groups):
    """``J``: ``min(n, DEFAULT_GROUPS)`` for ``None``; ``ValueError`` for ``J > n`` or a replicate of fewer than 2 rows."""
    check_groups_type(name, n_groups)
    J = min(n, DEFAULT_GROUPS) if n_groups is None else int(n_groups)
    if J > n:
        raise ValueError(f"{name} must not exceed the number of samples, got {J} with n = {n}")
    if J < 2 or n - -(-n // J) < 2:
        raise ValueError(f"{name} = {J} leaves a replicate of fewer than 2 of the {n} samples")
    return J


def check_limits(n, p, n_groups):
    """``ValueError`` for what the device path excludes, before the device is touched."""
    check_groups_type("n_groups", n_groups)
    _resample.check_shape("jackknife", n, p)
    resolve_groups("n_groups", n, n_groups)


def groups(n, n_groups):
    """The rows each replicate leaves out: group ``g`` is ``g, g + J, g + 2 J, ...``."""
    return [np.arange(g, n, n_groups) for g in range(n_groups)]


def jack_rcca(h, n, p1, p2, x1_ptr, x2_ptr, n_groups, g0, ng, c1, c2, center, k, sv_ptr, w_ptr, info_ptr):
    """One ``ccz_jack_rcca`` call (enqueue-only): replicates ``[g0, g0 + ng)`` of ``n_groups``."""
    vp = C.c_void_p
    h.check(h.lib.ccz_jack_rcca(h.raw, int(n), int(p1), int(p2), vp(int(x1_ptr)), vp(int(x2_ptr)), int(n_groups), int(g0), int(ng),
                                float(c1), float(c2), int(bool(center)), int(k), vp(int(sv_ptr)), vp(int(w_ptr)), vp(int(info_ptr))))


def run_replicates(h, n, p, zptr, c_, center, k, n_groups):
    """All ``J`` replicates on the (shifted) float64 device views ``zptr``: host ``(sv (J, r), W (J, p1 + p2, k), info (J,))``."""
    J, r, pt = int(n_groups), min(p), p[0] + p[1]
    sv, W, info = h.alloc(J * r * 8), h.alloc(J * pt * k * 8), h.alloc(J * 4)
    jack_rcca(h, n, p[0], p[1], zptr[0], zptr[1], J, 0, J, c_[0], c_[1], center, k, sv.ptr, W.ptr, info.ptr)
    return h.to_host(sv, (J, r)), h.to_host(W, (J, pt, k)), h.to_host(info, (J,), dtype=np.int32)


def raise_for_info(info, name="jackknife"):
    """``np.linalg.LinAlgError`` for the first non-zero ``info`` (``info[g]``: replicate g)."""
    for g in np.flatnonzero(info):
        code = int(info[g])
        raise np.linalg.LinAlgError(f"{name}: replicate {g}: {_bootstrap.INFO_CAUSES.get(code, f'info = {code}')}")


def summaries(jack, theta_hat):
    """``(se, bias)`` of the delete-group jackknife: ``sqrt((J - 1) / J * sum_g (theta_g - mean)^2)`` and ``(J - 1) (mean - theta_hat)``."""
    jack = np.asarray(jack, dtype=np.float64)
    J = jack.shape[0]
    mean = jack.mean(axis=0)
    return np.sqrt((J - 1) / J * np.sum((jack - mean) ** 2, axis=0)), (J - 1) * (mean - np.asarray(theta_hat, dtype=np.float64))


def bca_intervals(theta_hat, boot, jack, confidence_level):
    r"""Bias-corrected and accelerated bootstrap intervals, vectorised over any trailing shape.

    Args:
        theta_hat: the observed statistic, shape ``S``.
        boot: its bootstrap values, ``(B,) + S``.
        jack: its jackknife values, ``(J,) + S``.
        confidence_level: in (0, 1).

    Returns:
        ``(ci, z0, a)`` with ``ci`` of shape ``(2,) + S`` and ``z0``, ``a`` of shape ``S``, by the rule of ``scipy.stats.bootstrap``:

            z0 = Phi^-1((#{boot < theta_hat} + #{boot <= theta_hat}) / (2 B))
            a = sum d^3 / (6 (sum d^2)^(3/2)),   d = mean(jack) - jack
            alpha_-+ = Phi(z0 + (z0 -+ z) / (1 - a (z0 -+ z))),   z = Phi^-1((1 + confidence_level) / 2)
            ci = quantile(boot, [alpha_-, alpha_+]) per entry.

        Where ``z0`` is infinite (``theta_hat`` lies outside the bootstrap values) or ``sum d^2 = 0`` (a constant jackknife) the
        entry's interval is NaN, and one ``RuntimeWarning`` says how many entries; scipy does the same.
    """
    from scipy.special import ndtr, ndtri

    theta_hat = np.asarray(theta_hat, dtype=np.float64)
    boot, jack = np.asarray(boot, dtype=np.float64), np.asarray(jack, dtype=np.float64)
    if boot.shape[1:] != theta_hat.shape or jack.shape[1:] != theta_hat.shape:
        raise ValueError(f"boot {boot.shape} and jack {jack.shape} must be (B,) + S and (J,) + S with S = {theta_hat.shape}")
    B = boot.shape[0]
    with np.errstate(divide="ignore", invalid="ignore"):
        z0 = ndtri((np.sum(boot < theta_hat, axis=0) + np.sum(boot <= theta_hat, axis=0)) / (2.0 * B))
        d = jack.mean(axis=0) - jack
        a = np.sum(d ** 3, axis=0) / (6.0 * np.sum(d ** 2, axis=0) ** 1.5)
        z = float(ndtri((1.0 + confidence_level) / 2.0))
        alpha = np.stack([ndtr(z0 + (z0 + sz) / (1.0 - a * (z0 + sz))) for sz in (-z, z)])
    bad = ~(np.isfinite(z0) & np.isfinite(a) & np.all(np.isfinite(alpha), axis=0))
    ci = np.full((2,) + theta_hat.shape, np.nan)
    flat_ci, flat_alpha, flat_boot = ci.reshape(2, -1), alpha.reshape(2, -1), boot.reshape(B, -1)
    for e in np.flatnonzero(~bad.reshape(-1)):
        flat_ci[:, e] = np.quantile(flat_boot[:, e], flat_alpha[:, e])
    if np.any(bad):
        warnings.warn(f"bca_intervals: {int(np.sum(bad))} of {bad.size} intervals are NaN: the observed value lies outside the "
                      "bootstrap values, or the jackknife values are all equal", RuntimeWarning, stacklevel=2)
    return ci, z0, a


def jackknife(estimator, views, n_groups=None):
    r"""Delete-group jackknife of the weights and singular values of a two-view CCA, rCCA or PLS.

    Replicate ``g`` of ``J = n_groups`` is the fit on all rows except those with ``s % J == g``; every replicate is refitted on
    the device from the full-sample moments minus the moments of its group (see the module docstring).  The observed values
    come from the same device path on all rows.

    Args:
        estimator: an unfitted :class:`~cca_zoo_amd.linear.CCA`, :class:`~cca_zoo_amd.linear.rCCA` or
            :class:`~cca_zoo_amd.linear.PLS` (or a subclass of ``rCCA``), as for
            :func:`~cca_zoo_amd.model_selection.bootstrap`; the object itself is not changed (a clone is fitted).
        views: two (n, p_i) host ``float32`` / ``float64`` arrays, or two 2-D CUDA tensors of those dtypes.
        n_groups: ``J``.  ``None`` (default) means ``min(n, DEFAULT_GROUPS)`` with ``DEFAULT_GROUPS = 4096`` -- a documented
            default, not a measured optimum.  Pass ``n_groups=n`` for leave-one-out.

    Returns:
        :class:`JackknifeResult`.  ``se = sqrt((J - 1) / J * sum_g (theta_g - mean)^2)``, ``bias = (J - 1) (mean - observed)``:
        the formulas for groups of equal size, used also when ``J`` does not divide ``n`` (the group sizes then differ by one).
        Signs are those of ``bootstrap``: the observed columns by their largest stacked entry, each replicate aligned with the
        observed column.

    Limits (``ValueError`` before the device is touched): those of ``bootstrap`` (``max(p1, p2) <= 64``, ``n < 2^31``, ``n >= 2``);
    ``n_groups`` an integer with ``2 <= n_groups <= n`` that leaves every replicate at least 2 rows
    (``n - ceil(n / n_groups) >= 2``).  Sparse views and half-precision views raise ``TypeError``; a call inside
    :func:`cca_zoo_amd.row_sharded` raises ``NotImplementedError``.  A replicate whose regularised covariance cannot be
    factored raises ``np.linalg.LinAlgError`` that names the replicate and the remedy ``c > 0``.
    """
    est, views_, n, p, c_, center, on_device = _resample.prepare(
        "jackknife", "refits on all rows of one device", estimator, views, lambda n, p: check_limits(n, p, n_groups))
    J = resolve_groups("n_groups", n, n_groups)
    r = min(p)
    k, pt = min(int(est.latent_dimensions), r), p[0] + p[1]

    h = _backend.handle_for(views_)
    x64, xptr = _resample.stage_f64(h, views_, on_device)  # for the column means and the shift
    sp = acquire(h, views_)
    try:
        Z = [_bootstrap._shifted(h, xptr[i], n, p[i], center) for i in range(2)]
        zptr = [int(z.ptr) if z is not None else xptr[i] for i, z in enumerate(Z)]
        sv, W, info = h.alloc(r * 8), h.alloc(pt * k * 8), h.alloc(4)
        _bootstrap.boot_rcca(h, n, p[0], p[1], zptr[0], zptr[1], None, 1, c_[0], c_[1], center, k, sv.ptr, W.ptr, info.ptr)
        sv_j, W_j, info_j = run_replicates(h, n, p, zptr, c_, center, k, J)
        sv_h, W_h = h.to_host(sv, (1, r)), h.to_host(W, (1, pt, k))
        info_h = h.to_host(info, (1,), dtype=np.int32)
    finally:
        release(h, sp)
    del x64, Z
    if info_h[0]:
        raise np.linalg.LinAlgError(f"jackknife: the observed sample: {_bootstrap.INFO_CAUSES.get(int(info_h[0]), f'info = {int(info_h[0])}')}")
    raise_for_info(info_j)
    if not (np.all(np.isfinite(sv_h)) and np.all(np.isfinite(W_h)) and np.all(np.isfinite(sv_j)) and np.all(np.isfinite(W_j))):
        raise np.linalg.LinAlgError("jackknife: the replicates' solutions are not finite")
    W_obs = _bootstrap.orient_observed(W_h[0])
    W_jack = _bootstrap.orient_to(W_j, W_obs)
    sv_se, sv_bias = summaries(sv_j, sv_h[0])
    w_se, w_bias = summaries(W_jack, W_obs)
    cut = [slice(0, p[0]), slice(p[0], pt)]
    est.fit(list(views))
    return JackknifeResult(singular_values=sv_h[0].copy(), weights=[W_obs[s].copy() for s in cut], singular_values_jack=sv_j,
                           weights_jack=[np.ascontiguousarray(W_jack[:, s]) for s in cut], singular_values_se=sv_se,
                           weights_se=[w_se[s].copy() for s in cut], singular_values_bias=sv_bias,
                           weights_bias=[w_bias[s].copy() for s in cut], n_groups=J, estimator=est)
