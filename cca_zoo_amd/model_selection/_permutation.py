"""permutation_test -- the row-permutation null of the two-view canonical correlations, whole permutations on the device.

The reference has no counterpart: there, as with the estimators here, the test is a Python loop of ``B`` refits on
``[X1, X2[pi]]``.  A row permutation of view 2 leaves both means and both covariances as they are -- only the cross block
changes -- so both views are whitened once,

    R_i = (1 - c_i) C_ii + c_i I = L_i L_i',     Z_i = (X_i - 1 mu_i') L_i^-T,

and permutation ``pi`` has the singular values of ``Z_1' Z_2[pi] / (n - 1)``: canonical correlations for ``c = 0``,
covariances for ``PLS``.  ``tests/perm_restatement.py`` is the float64 NumPy form the device is held to.

Device side: one float64 K1 pass per view (``ccz_moments``), ``ccz_cholinv`` for both ``L_i^-1``, ``ccz_transform`` in float64 for
``Z_i``, then ``ccz_perm_singular_values`` (``csrc/perm.hip``): a gathered cross-moment product on the fp64 matrix pipe and a
one-sided Jacobi SVD, many permutations per launch.  The host draws the permutations with NumPy, one chunk ahead of the device
(``_resample.py``, shared with :func:`~cca_zoo_amd.model_selection.bootstrap`); with ``draws="device"`` they are drawn on the
device instead (``ccz_draw_permutations``, ``csrc/draw.hip``: the argsort of hashed 64-bit keys), straight into the slot the
product reads.
"""

from __future__ import annotations

import ctypes as C
from dataclasses import dataclass
from numbers import Integral
from typing import Any

import numpy as np

from cca_zoo_amd import _backend
from cca_zoo_amd._utils._resident import acquire, release
from cca_zoo_amd.model_selection import _resample
from cca_zoo_amd.model_selection._resample import MAX_ROWS, MAX_WIDTH, ROWS_PER_SPLIT  # noqa: F401  (the limits, for callers)

#: permutations per upload and ``ccz_perm_singular_values`` call (fewer when a chunk's indices would exceed
#: ``CHUNK_INDEX_BYTES``); the result does not depend on it by a bit
CHUNK_PERMS = 64
CHUNK_INDEX_BYTES = 64 << 20


@dataclass
class PermutationTestResult:
    """What :func:`permutation_test` returns; ``r = min(p1, p2)``, ``B = n_permutations``."""

    statistic: np.ndarray       # (r,)   observed singular values, descending
    null: np.ndarray            # (B, r) the same for each permutation of the rows of view 2
    pvalues: np.ndarray         # (r,)   (1 + #{b : null[b, j] >= statistic[j]}) / (B + 1)
    tail: np.ndarray            # (r,)   tail[j] = sum_{i >= j} statistic[i]^2
    tail_null: np.ndarray       # (B, r)
    tail_pvalues: np.ndarray    # (r,)   the same counting rule on the tails; tail_pvalues[0] is the omnibus test
    estimator: Any              # the estimator fitted on the unpermuted views


def draw_permutations(rng, n, count):
    """``count`` x ``n`` row indices (int32), one ``rng.permutation(n)`` per row, in order."""
    out = np.empty((count, n), dtype=np.int32)
    for b in range(count):
        out[b] = rng.permutation(n)
    return out


def permutation_chunks(rng, n, total, chunk):
    """The ``total`` permutations of :func:`draw_permutations` in chunks of at most ``chunk``, drawn as they are asked for."""
    return _resample.chunks(draw_permutations, rng, n, total, chunk)


def chunk_length(n):
    """Permutations per upload: ``CHUNK_PERMS``, fewer when their indices would exceed ``CHUNK_INDEX_BYTES``."""
    return _resample.chunk_length(n, CHUNK_PERMS, CHUNK_INDEX_BYTES)


def tails(sv):
    """``tail[..., j] = sum_{i >= j} sv[..., i]^2`` (Pillai-type tail of the squared singular values)."""
    sq = np.asarray(sv, dtype=np.float64) ** 2
    return np.cumsum(sq[..., ::-1], axis=-1)[..., ::-1]


def count_pvalues(statistic, null):
    """``(1 + #{b : null[b, j] >= statistic[j]}) / (B + 1)`` per column."""
    null = np.asarray(null)
    return (1.0 + np.sum(null >= np.asarray(statistic)[None, :], axis=0)) / (null.shape[0] + 1.0)


def check_limits(n, p, n_permutations):
    """``ValueError`` for what the device path excludes, before the device is touched."""
    if isinstance(n_permutations, bool) or not isinstance(n_permutations, Integral) or n_permutations < 1:
        raise ValueError(f"n_permutations must be an integer >= 1, got {n_permutations!r}")
    _resample.check_shape("permutation_test", n, p, ", as is customary for permutation inference")


def _whiten(h, xptr, n, d, c, center):
    """``(X - 1 mu') L^-T`` of one device float64 view as a device buffer; ``R = (1 - c) C + c I = L L'``."""
    mom = h.alloc((d * d + d) * 8)
    h.moments([(xptr, d, d)], n, _backend.F64, True, mom.ptr, pilot=False, timed=False)
    h.moments_symmetrize(mom.ptr, d)
    flat = h.to_host(mom, (d * d + d,))
    G, s = flat[: d * d].reshape(d, d), flat[d * d:]
    if not np.all(np.isfinite(s)) or not np.all(np.isfinite(G)):
        raise ValueError("Input contains NaN or infinity.")
    mean = s / n
    cov = (G - np.outer(s, mean) if center else G) / (n - 1)
    R = (1.0 - c) * 0.5 * (cov + cov.T) + c * np.eye(d)
    vp = C.c_void_p
    a_d, l_d, x_d = h.to_device(R), h.alloc(d * d * 8), h.alloc(d * d * 8)
    h.memset0(x_d.ptr, d * d * 8)
    h.check(h.lib.ccz_cholinv(h.raw, 1, (vp * 1)(a_d.ptr), (C.c_int64 * 1)(d), (vp * 1)(l_d.ptr), (vp * 1)(x_d.ptr)))
    w_d = h.to_device(np.ascontiguousarray(np.tril(h.to_host(x_d, (d, d))).T))     # L^-T (d x d; never a view)
    mu_d = h.to_device(mean) if center else None
    z_d = h.alloc(n * d * 8)
    h.check(h.lib.ccz_transform(h.raw, _backend.F64, vp(xptr), n, d, d, vp(mu_d.ptr) if mu_d else None, vp(w_d.ptr), d,
                                vp(z_d.ptr), d))
    return z_d, (w_d, mu_d)


def singular_values(h, n, p1, p2, z1_ptr, z2_ptr, perms_ptr, nperm, sv_ptr):
    """One ``ccz_perm_singular_values`` call (enqueue-only); ``perms_ptr`` None = the identity."""
    vp = C.c_void_p
    h.check(h.lib.ccz_perm_singular_values(h.raw, int(n), int(p1), int(p2), vp(int(z1_ptr)), vp(int(z2_ptr)),
                                           vp(int(perms_ptr)) if perms_ptr else None, int(nperm), 1.0 / (n - 1), vp(int(sv_ptr))))


def permutation_test(estimator, views, n_permutations=1000, random_state=None, *, draws="numpy"):
    r"""Row-permutation test of the canonical correlations of two views.

    The rows of view 2 are shuffled ``n_permutations`` times; every shuffle gives all ``r = min(p1, p2)`` singular values
    of the whitened cross-covariance, computed on the device without refitting (see the module docstring).  The
    observed values (``statistic``) come from the same device path with the identity permutation.

    Args:
        estimator: an unfitted :class:`~cca_zoo_amd.linear.CCA`, :class:`~cca_zoo_amd.linear.rCCA` or
            :class:`~cca_zoo_amd.linear.PLS` (or a subclass of ``rCCA``); its ridge ``c`` and ``center`` define the
            statistic.  ``latent_dimensions`` only affects the returned fitted estimator: the test always returns all
            ``r`` values.  The object itself is not changed (a clone is fitted).
        views: two (n, p_i) host ``float32`` / ``float64`` arrays, or two 2-D CUDA tensors of those dtypes.  float32 views
            are widened to float64 once; every product after that is float64.
        n_permutations: ``B >= 1``.
        random_state: seed of ``np.random.default_rng``; permutation ``b`` is the ``b``-th ``rng.permutation(n)``.
        draws: ``"numpy"`` (default): the permutations are drawn on the host as above and uploaded.  ``"device"``: they are
            drawn on the device and no index array is built or uploaded by the host -- permutation ``b`` is the argsort of the
            ``n`` keys ``splitmix64(stream(seed, b) ^ splitmix64(j))`` (``include/ccz.h``: ``ccz_draw_permutations``) with
            ``seed = np.random.default_rng(random_state).integers(0, 2**64, dtype=np.uint64)``.  The two settings give
            different, equally valid random permutations: ``statistic`` is the same bits, ``null`` and the p-values differ by
            Monte Carlo error only.  Either setting is reproducible from ``random_state``.

    Returns:
        :class:`PermutationTestResult`.

    Limits of this first cut (``ValueError`` before the device is touched): ``max(p1, p2) <= 64`` -- wider views are
    reduced first (e.g. to their leading principal components), as is customary for permutation inference; ``n < 2^31``;
    ``n >= 2``; ``draws`` is one of the two names.  Sparse views and half-precision views raise ``TypeError``; a call inside
    :func:`cca_zoo_amd.row_sharded` raises ``NotImplementedError``.

    ``pvalues[j]`` for ``j > 0`` is the plain comparison of the ``j``-th order statistic with its permutation
    distribution.  It is NOT a stepwise (deflating) test: the null of component ``j`` still contains the signal of the
    components before it.  ``tail_pvalues[0]`` (all squared singular values summed) is the omnibus test.
    """
    est, views_, n, p, c_, center, on_device = _resample.prepare(
        "permutation_test", "whitens all rows on one device", estimator, views, lambda n, p: check_limits(n, p, n_permutations),
        draws)
    B, r = int(n_permutations), min(p)

    h = _backend.handle_for(views_)
    x64, xptr = _resample.stage_f64(h, views_, on_device)  # for K1 and the whitening
    sp = acquire(h, views_)
    try:
        Z, keep = [], []
        for i in range(2):
            z, k = _whiten(h, xptr[i], n, p[i], c_[i], center)
            Z.append(z), keep.append(k)
        sv = h.alloc((B + 1) * r * 8)
        singular_values(h, n, p[0], p[1], Z[0].ptr, Z[1].ptr, None, 1, sv.ptr)
        chunk = chunk_length(n)
        if draws == "device":
            source = _resample.device_chunks(h, "permutations", n, _resample.device_seed(random_state), B, chunk)
        else:
            source = permutation_chunks(np.random.default_rng(random_state), n, B, chunk)
        slots = _resample.run_chunks(h, source, min(chunk, B) * n * 4,
                                     lambda ptr, count, done: singular_values(h, n, p[0], p[1], Z[0].ptr, Z[1].ptr, ptr, count,
                                                                              sv.ptr + (1 + done) * r * 8))
        out = h.to_host(sv, (B + 1, r))
    finally:
        release(h, sp)
    del x64, keep, Z, slots
    if not np.all(np.isfinite(out)):
        raise np.linalg.LinAlgError("permutation_test: the singular values are not finite")
    statistic, null = out[0].copy(), out[1:].copy()
    tail, tail_null = tails(statistic), tails(null)
    est.fit(list(views))
    return PermutationTestResult(statistic=statistic, null=null, pvalues=count_pvalues(statistic, null), tail=tail,
                                 tail_null=tail_null, tail_pvalues=count_pvalues(tail, tail_null), estimator=est)
