"""TCCA -- tensor canonical correlation analysis: whitening, cross-moment tensor and CP-ALS on the device.

Reference: ``cca_zoo/linear/_tcca.py``.  Per view the covariance comes out of one float64 K1 pass (``ccz_moments``), its inverse
square root from the device Jacobi EVD (``ccz_syevj``; ``V diag(lam^-1/2) V'`` as two ``ccz_gemm_f64``), the whitened view
``H_i = X_i cov_i^-1/2`` from ``ccz_transform`` in float64.  ``ccz_kr_moment`` builds ``M = (1 / n) sum_s H_1[s] (x) .. (x)
H_V[s]`` without the reference's ``n x p_1 x .. x p_V`` array, and ``csrc/cp_als.hip`` decomposes it: whole CP-ALS
iterations on the device, enqueued in chunks behind a device stop word.

The factor step is NOT tensorly's code: tensorly is not a dependency, so the algorithm that its documented ``parafac``
defaults describe is written out (``include/ccz.h``; ``tests/tcca_fit_restatement.py`` is the NumPy form the device is
held to).  The whitening, the tensor and ``weights_[i] = cov_i^-1/2 A_i`` follow the reference.
"""

from __future__ import annotations

import ctypes as C
from numbers import Integral
from typing import Any, ClassVar

import numpy as np
from sklearn.utils._param_validation import Interval

from cca_zoo_amd import _backend
from cca_zoo_amd._base import BaseModel
from cca_zoo_amd._utils._param_constraints import POSITIVE_EPS, RIDGE_PARAMETER
from cca_zoo_amd._utils._resident import acquire, as_float, fit_state, is_f32, refuse_row_sharded, release, run_chunks
from cca_zoo_amd._utils._validation import is_device_tensor, perview_parameter

#: iterations per ``ccz_cp_iterations`` call (one host wait per chunk, for the chunk two calls back)
CHUNK_ITERS = 16
#: tensorly's ``parafac`` defaults, with which the reference calls it
N_ITER_MAX, TOL = 100, 1e-8
#: limits of the device path (``csrc/cp_als.hip``, ``csrc/krmoment.hip``)
MAX_DIMS, MAX_VIEWS, MAX_ENTRIES = 32, 8, 1 << 24
_CP_SINGULAR = 3


def check_tensor_limits(name, k, widths):
    """``ValueError`` for what the device path excludes, before the device is touched."""
    m = len(widths)
    if m < 2 or m > MAX_VIEWS:
        raise ValueError(f"{name}: 2 to {MAX_VIEWS} views are supported, got {m}")
    if k > min(MAX_DIMS, min(widths)):
        raise ValueError(f"{name}: latent_dimensions={k} exceeds min({MAX_DIMS}, narrowest tensor mode = {min(widths)}); the "
                         "SVD initialisation has no more columns (tensorly would pad it with random ones)")
    prod = 1
    for w in widths:
        prod *= int(w)
    if prod > MAX_ENTRIES:
        raise ValueError(f"{name}: the cross-moment tensor would have {prod} entries, the limit is 2^24")


def inv_sqrt_shifted(h, cov, eps):
    """``(cov + shift I)^-1/2`` with the reference's ``shift = eps - min_eig`` when the smallest eigenvalue is below eps
    (``_tcca.py:140-146``): the EVD on the device, ``V diag(lam^-1/2) V'`` as a device product.  ``cov``: host float64.
    Returns the result as a device buffer (d x d) and as a host array."""
    d = int(cov.shape[0])
    cov = np.ascontiguousarray(cov, dtype=np.float64)
    if not np.all(np.isfinite(cov)):
        raise ValueError("Input contains NaN or infinity.")
    if d == 1:
        lam, Vr = cov.reshape(1).copy(), np.ones((1, 1))
    else:
        a, w, vr = h.to_device(cov), h.alloc(d * 8), h.alloc(d * d * 8)
        h.check(h.lib.ccz_syevj(h.raw, C.c_void_p(a.ptr), d, C.c_void_p(w.ptr), C.c_void_p(vr.ptr), None))
        lam, Vr = h.to_host(w, (d,)), h.to_host(vr, (d, d))      # row i = eigenvector i
    if lam.min() < eps:
        lam = lam + (eps - lam.min())
    if not lam.min() > 0:
        raise np.linalg.LinAlgError("the regularised covariance is not positive definite")
    vd, sd = h.to_device(Vr), h.to_device(Vr / np.sqrt(lam)[:, None])
    F = h.alloc(d * d * 8)
    h.gemm(True, False, d, d, d, 1.0, vd.ptr, d, sd.ptr, d, 0.0, F.ptr, d)
    return F, h.to_host(F, (d, d))


def decompose(h, H_ptrs, widths, n, k):
    """The cross-moment tensor of the whitened views (device float64, ``n x widths[i]`` row-major) and its CP-ALS.
    Returns (factors, error trace); a singular update raises ``LinAlgError`` as the reference's ``solve`` would."""
    m = len(widths)
    prod = int(np.prod(widths, dtype=np.int64))
    varr = (_backend.View * m)()
    for i, (ptr, w) in enumerate(zip(H_ptrs, widths)):
        varr[i].data, varr[i].cols, varr[i].ld = int(ptr), int(w), int(w)
    M = h.alloc(prod * 8)
    h.check(h.lib.ccz_kr_moment(h.raw, varr, m, int(n), 1.0 / n, C.c_void_p(M.ptr)))
    pd = C.POINTER(C.c_double)
    with fit_state(h, "cp", m, (C.c_int64 * m)(*[int(w) for w in widths]), int(k), TOL, N_ITER_MAX, CHUNK_ITERS) as state:
        h.check(h.lib.ccz_cp_setup(h.raw, state, C.c_void_p(M.ptr)))
        known, stopped = C.c_int64(-1), C.c_int(0)

        def iterations(step):
            h.check(h.lib.ccz_cp_iterations(h.raw, state, step, C.byref(known), C.byref(stopped)))
            return stopped.value

        run_chunks(N_ITER_MAX, CHUNK_ITERS, iterations)
        iters, stop, reason = C.c_int64(0), C.c_int(0), C.c_int(0)
        h.check(h.lib.ccz_cp_status(h.raw, state, C.byref(iters), C.byref(stop), C.byref(reason), None, None))
        if reason.value == _CP_SINGULAR:
            raise np.linalg.LinAlgError(f"CP-ALS: singular matrix in the update of iteration {iters.value}")
        if not stop.value:
            raise RuntimeError(f"CP-ALS ended after {iters.value} of {N_ITER_MAX} iterations")   # cannot happen
        flat, trace = np.empty(sum(widths) * k), np.empty(N_ITER_MAX)
        h.check(h.lib.ccz_cp_get_result(h.raw, state, flat.ctypes.data_as(pd), trace.ctypes.data_as(pd), C.byref(iters)))
    offs = np.cumsum([0] + [int(w) * k for w in widths])
    factors = [flat[offs[i]:offs[i + 1]].reshape(int(w), k).copy() for i, w in enumerate(widths)]
    if not all(np.all(np.isfinite(a)) for a in factors):
        raise np.linalg.LinAlgError("CP-ALS: the factors are not finite")
    return factors, trace[:iters.value].copy()


class TCCA(BaseModel):
    r"""Tensor CCA (Kim, Wong & Cipolla 2007; Luo et al. 2015): the rank-k CP decomposition of the cross-moment tensor of
    the whitened views.

    Fitted attributes: ``weights_`` (float64, ``p_i x latent_dimensions``), ``means_``; not in the reference: ``n_iter_``
    (CP-ALS iterations) and ``rec_error_`` (the relative reconstruction error after every iteration).

    Differences from the reference, on purpose:

    - 2 to 8 views, ``prod p_i <= 2^24``, ``latent_dimensions <= min(32, min p_i)`` (``ValueError`` otherwise).
    - ``fit`` inside :func:`cca_zoo_amd.row_sharded` raises ``NotImplementedError``.
    - float32 views are widened to float64 once and every product after that is float64 (the reference
      centres in float32 and promotes in ``np.cov``).  The float32 K1 product was tried for the covariance and measured
      two to three times the reference's own float32-to-float64 gap, which is the bar these fits are held to.
    - The decomposition is the CP-ALS stated in ``include/ccz.h`` (tensorly's documented defaults), not tensorly's code;
      it is deterministic and ``random_state`` is accepted and unused.

    As in the reference, ``np.cov`` always subtracts the mean: with ``center=False`` the covariance is still the centred
    one while the whitening multiplies the views as given.

    Args:
        latent_dimensions: Number of latent dimensions. Default is 1.
        center: Whether to subtract column means before fitting. Default True.
        c: Ridge regularisation in ``[0, 1]`` (scalar or one per view). Default is 0.
        eps: Floor of the smallest eigenvalue of every regularised covariance. Default is 1e-6.
        random_state: Accepted for compatibility; unused.
    """

    _parameter_constraints: ClassVar[dict[str, list[Any]]] = {
        **BaseModel._parameter_constraints,
        "c": RIDGE_PARAMETER,
        "eps": POSITIVE_EPS,
        "random_state": [None, Interval(Integral, 0, None, closed="left")],
    }

    def __init__(self, latent_dimensions: int = 1, center: bool = True, c: float | list[float] = 0.0, eps: float = 1e-6,
                 random_state: int | None = None) -> None:
        super().__init__(latent_dimensions=latent_dimensions, center=center)
        self.c = c
        self.eps = eps
        self.random_state = random_state

    def fit(self, views, y=None):
        """Fit to a list of (n_samples, n_features_i) host arrays or CUDA tensors."""
        refuse_row_sharded("TCCA decomposes one cross-moment tensor of all rows, which this build does not shard by rows")
        views_ = [as_float(v) for v in self._setup_fit(views)]
        m, n, p = self.n_views_, self.n_samples_, self.n_features_in_
        k = int(self.latent_dimensions)
        c_ = [float(v) for v in perview_parameter("c", self.c, 0.0, m)]
        check_tensor_limits("TCCA", k, p)
        if n < 2:
            raise ValueError("at least 2 samples are required")
        dev = [is_device_tensor(v) for v in views_]
        if any(dev) and not all(dev):
            raise ValueError("views must be all host arrays or all CUDA tensors")
        f32 = all(is_f32(v) for v in views_)
        h = _backend.handle_for(views_)
        # float64 copies for K1 and the whitening, made before the handle's stream takes over (CUDA: on the caller's stream)
        if all(dev):
            import torch

            x64 = [v.to(torch.float64).contiguous() for v in views_]
            xptr = [int(x.data_ptr()) for x in x64]
        else:
            x64 = [h.to_device(np.ascontiguousarray(v, dtype=np.float64)) for v in views_]
            xptr = [int(b.ptr) for b in x64]
        sp = acquire(h, views_)
        try:
            F_host, H, means, keep = [], [], [], []
            for i, v in enumerate(views_):
                d = p[i]
                mom = h.alloc((d * d + d) * 8)
                h.moments([(xptr[i], d, d)], n, _backend.F64, True, mom.ptr, pilot=False, timed=False)
                h.moments_symmetrize(mom.ptr, d)
                flat = h.to_host(mom, (d * d + d,))
                G, s = flat[: d * d].reshape(d, d), flat[d * d:]
                if not np.all(np.isfinite(s)):
                    raise ValueError("Input contains NaN or infinity.")
                mean = s / n
                cov = (1.0 - c_[i]) * (G - np.outer(s, mean)) / (n - 1) + c_[i] * np.eye(d)     # np.cov: always centred
                Fd, Fh = inv_sqrt_shifted(h, 0.5 * (cov + cov.T), float(self.eps))
                mu = h.to_device(mean) if self.center else None
                Hd = h.alloc(n * d * 8)
                h.check(h.lib.ccz_transform(h.raw, _backend.F64, C.c_void_p(xptr[i]), n, d, d, C.c_void_p(mu.ptr) if mu else None,
                                            C.c_void_p(Fd.ptr), d, C.c_void_p(Hd.ptr), d))
                F_host.append(Fh), H.append(Hd), means.append(mean if self.center else np.zeros(d)), keep.append((Fd, mu))
            factors, trace = decompose(h, [b.ptr for b in H], p, n, k)
        finally:
            release(h, sp)
        del x64, keep, H
        self._store([f @ a for f, a in zip(F_host, factors)], means, "f32" if f32 else "f64", weights_like_input=False)
        self.n_iter_ = int(trace.size)
        self.rec_error_ = trace
        return self
