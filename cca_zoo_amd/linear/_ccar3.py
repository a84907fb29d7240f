"""CCAR3 -- canonical correlation analysis as reduced-rank regression: everything from the second moments, the ADMM
iterations on the device.

Reference: ``cca_zoo/linear/_ccar3.py``.  One float64 K1 pass (``ccz_moments``) over ``[X Y]`` gives ``Sxx``, ``Sxy`` and
``Syy`` (``ccz_moments_block``: division by n, centred when ``center``); sklearn's Ledoit-Wolf shrinkage of the ``Y``
covariance needs one more scalar, ``sum_i |y_i - ybar|^4`` (``ccz_rownorm4``, one streaming pass over ``Y``).  ``R = Sy^-1/2``
comes from the device Jacobi EVD (``ccz_syevj``) with the eigenvalues up to 1e-4 zeroed, ``P = Sxy R`` from ``ccz_gemm_f64``.
``highdim=True``: ``M = (Sxx + (rho + eps) I)^-1`` is formed once (``ccz_cholinv`` and one product) and ``csrc/rrr.hip`` runs
whole ADMM iterations on the device, enqueued in chunks behind a device stop word.  ``highdim=False``: factor and two
triangular solves.  The SVD of the coefficient matrix is ``ccz_gesvj``; the ``r x r`` whitening factors, signs, order and
padding are formed on the host.  ``tests/ccar3_restatement.py`` is the NumPy form the device is held to.
"""

from __future__ import annotations

import ctypes as C
from numbers import Real
from typing import Any, ClassVar

import numpy as np
from sklearn.utils._param_validation import Interval

from cca_zoo_amd import _backend
from cca_zoo_amd._base import BaseModel
from cca_zoo_amd._utils._param_constraints import POSITIVE_EPS, POSITIVE_INT
from cca_zoo_amd._utils._resident import acquire, as_float, fit_state, is_f32, refuse_row_sharded, release, run_chunks
from cca_zoo_amd._utils._validation import is_device_tensor

#: iterations per ``ccz_rrr_iterations`` call (one host wait per chunk, for the chunk two calls back)
CHUNK_ITERS = 16
#: limits of the device path (``csrc/rrr.hip``): ``p + q`` is the largest width the moments path has been run at, and one
#: workgroup holds a whole row of the coefficient matrix
MAX_FEATURES, MAX_Q = 16384, 1024
#: eigenvalues of the ``Y`` covariance up to this are zeroed in its inverse square root (the reference's ``_sqrt_inv_psd``)
CUT = 1e-4


def check_limits(p, q):
    """``ValueError`` for what the device path excludes, before the device is touched."""
    if p + q > MAX_FEATURES:
        raise ValueError(f"CCAR3: {p} + {q} features exceed the device path's limit of {MAX_FEATURES}")
    if q > MAX_Q:
        raise ValueError(f"CCAR3: the second view has {q} features, the device path supports at most {MAX_Q} "
                         "(swap the views to regularise the other one)")


def shrunk_covariance(cov, fourth, n):
    """sklearn's Ledoit-Wolf estimate from the centred covariance ``cov`` (division by n) and ``fourth = sum_i |y_i -
    ybar|^4``, the one quantity the second moments do not hold.  Returns (Sy, shrinkage)."""
    q = cov.shape[0]
    tr = np.trace(cov)
    mu = tr / q
    delta_ = np.sum(cov * cov)
    beta = (fourth / n - delta_) / (q * n)
    delta = (delta_ - 2.0 * mu * tr + q * mu * mu) / q
    beta = min(beta, delta)
    shrinkage = 0.0 if beta == 0 else beta / delta
    Sy = (1.0 - shrinkage) * cov
    Sy[np.diag_indices(q)] += shrinkage * mu
    return Sy, float(shrinkage)


def whiten_factor(G, eps):
    """W with ``W' G W = I``: the inverse transposed Cholesky factor of ``sym(G) + eps I``, or (the reference's fallback when
    that fails) the symmetric inverse square root with the eigenvalues raised to eps."""
    G = 0.5 * (G + G.T) + eps * np.eye(G.shape[0])
    try:
        return np.linalg.inv(np.linalg.cholesky(G)).T
    except np.linalg.LinAlgError:
        lam, V = np.linalg.eigh(G)
        return (V / np.sqrt(np.maximum(lam, eps))) @ V.T


def inv_sqrt_cut(h, Sy):
    """``V diag(lam^-1/2 where lam > CUT, else 0) V'``: the EVD on the device, the product as a device product.  Returns the
    result as a device buffer (q x q) and as a host array."""
    q = int(Sy.shape[0])
    Sy = np.ascontiguousarray(0.5 * (Sy + Sy.T))
    if not np.all(np.isfinite(Sy)):
        raise ValueError("Input contains NaN or infinity.")
    if q == 1:
        lam, Vr = Sy.reshape(1).copy(), np.ones((1, 1))
    else:
        a, w, vr = h.to_device(Sy), h.alloc(q * 8), h.alloc(q * q * 8)
        h.check(h.lib.ccz_syevj(h.raw, C.c_void_p(a.ptr), q, C.c_void_p(w.ptr), C.c_void_p(vr.ptr), None))
        lam, Vr = h.to_host(w, (q,)), h.to_host(vr, (q, q))      # row i = eigenvector i
    f = np.zeros(q)
    keep = lam > CUT
    f[keep] = 1.0 / np.sqrt(lam[keep])
    vd, sd = h.to_device(Vr), h.to_device(Vr * f[:, None])
    Rd = h.alloc(q * q * 8)
    h.gemm(True, False, q, q, q, 1.0, vd.ptr, q, sd.ptr, q, 0.0, Rd.ptr, q)
    return Rd, h.to_host(Rd, (q, q))


def admm(h, Minv_ptr, P_ptr, p, q, lambda_, rho, tol, max_iter):
    """The ADMM family of ``csrc/rrr.hip`` on device ``M`` and ``P``.  Returns (Z on the host, iterations done)."""
    with fit_state(h, "rrr", p, q, float(lambda_), float(rho), float(tol), int(max_iter), CHUNK_ITERS) as state:
        h.check(h.lib.ccz_rrr_setup(h.raw, state, C.c_void_p(Minv_ptr), C.c_void_p(P_ptr)))
        known, stopped = C.c_int64(-1), C.c_int(0)

        def iterations(step):
            h.check(h.lib.ccz_rrr_iterations(h.raw, state, step, C.byref(known), C.byref(stopped)))
            return stopped.value

        run_chunks(int(max_iter), CHUNK_ITERS, iterations)
        iters, stop = C.c_int64(0), C.c_int(0)
        h.check(h.lib.ccz_rrr_status(h.raw, state, C.byref(iters), C.byref(stop), None, None, None))
        if not stop.value:
            raise RuntimeError(f"ADMM ended after {iters.value} of {max_iter} iterations")   # cannot happen
        Z = np.empty((p, q))
        h.check(h.lib.ccz_rrr_get_result(h.raw, state, Z.ctypes.data_as(C.POINTER(C.c_double)), None))
    return Z, int(iters.value)


class CCAR3(BaseModel):
    r"""Canonical correlation analysis via reduced-rank regression (Donnat & Tuzhilina 2024, arXiv:2405.19539).

    ``Y`` is whitened by its (optionally Ledoit-Wolf shrunk) covariance and a coefficient matrix ``B`` relating ``X`` to the
    whitened ``Y`` is estimated: in closed form (``highdim=False``, ``B = (Sxx + eps I)^-1 Sxy Sy^-1/2``) or by the row-wise
    group-lasso-penalised regression ``min_B (1/n) |Y Sy^-1/2 - X B|_F^2 + lambda_ sum_j |B_j|_2`` solved by ADMM
    (``highdim=True``, the default), which drives whole rows of ``B`` (whole ``X`` features) to zero.  The rank-
    ``latent_dimensions`` SVD of ``B`` gives the directions, which are whitened to unit variance, sign-aligned to positive
    correlation and sorted.  Sparsity is induced in ``X`` only: swap the views to regularise the other one.

    Fitted attributes: ``weights_`` (float64, ``p_i x latent_dimensions``; columns beyond ``min(p, q)`` are zero),
    ``means_``; not in the reference: ``n_iter_`` (ADMM iterations; 0 with ``highdim=False``) and ``shrinkage_`` (the
    Ledoit-Wolf coefficient; 0 without it).  Reaching ``max_iter`` without
    convergence returns the current iterate silently, as the reference does.

    Differences from the reference, on purpose:

    - Exactly as the reference, 2 views; here also ``p + q <= 16384`` and ``q <= 1024`` (``ValueError`` otherwise).
    - ``fit`` inside :func:`cca_zoo_amd.row_sharded` raises ``NotImplementedError`` (what is missing is the all-reduce of
      the moments and of one scalar).
    - The ADMM multiplies by the explicit inverse ``(Sxx + (rho + eps) I)^-1``, formed once; the reference solves with the
      Cholesky factor every iteration.  The matrix's condition number is at most ``(lambda_max(Sxx) + rho) / rho``, so the
      two agree to rounding.
    - Every quantity but one comes from the second moments of one K1 pass; the views are not centred or whitened in
      memory.  float32 views are widened to float64 once and every product after that is float64 (the reference runs
      in float32 throughout).
    - Views may be host arrays or CUDA tensors (not a mixture).

    Args:
        latent_dimensions: Number of latent dimensions. Default is 1.
        center: Whether to subtract column means before fitting. Default True.
        lambda_: Row-group-lasso strength used when ``highdim=True``; 0 disables the penalty. Default is 0.
        highdim: ADMM-solved group-lasso regression (default) or the closed-form low-dimensional solution (``False``).
        ledoit_wolf: Whether to shrink the ``Y`` covariance by Ledoit-Wolf before inverting it. Default True.
        rho: ADMM step-size parameter. Default 1.0.
        max_iter: Maximum number of ADMM iterations. Default 10_000.
        tol: ADMM tolerance on the primal / dual residuals. Default 1e-4.
        eps: Small constant added to covariance matrices before inversion. Default 1e-8.
    """

    _parameter_constraints: ClassVar[dict[str, list[Any]]] = {
        **BaseModel._parameter_constraints,
        "lambda_": [Interval(Real, 0, None, closed="left")],
        "highdim": ["boolean"],
        "ledoit_wolf": ["boolean"],
        "rho": POSITIVE_EPS,
        "max_iter": POSITIVE_INT,
        "tol": POSITIVE_EPS,
        "eps": POSITIVE_EPS,
    }

    def __init__(self, latent_dimensions: int = 1, center: bool = True, lambda_: float = 0.0, highdim: bool = True,
                 ledoit_wolf: bool = True, rho: float = 1.0, max_iter: int = 10_000, tol: float = 1e-4, eps: float = 1e-8) -> None:
        super().__init__(latent_dimensions=latent_dimensions, center=center)
        self.lambda_ = lambda_
        self.highdim = highdim
        self.ledoit_wolf = ledoit_wolf
        self.rho = rho
        self.max_iter = max_iter
        self.tol = tol
        self.eps = eps

    def fit(self, views, y=None):
        """Fit to a list of exactly two (n_samples, n_features_i) host arrays or CUDA tensors."""
        refuse_row_sharded("CCAR3 needs the moments and one fourth-moment scalar of all rows, which this build does not all-reduce")
        views_ = [as_float(v) for v in self._setup_fit(views)]
        if self.n_views_ != 2:
            raise ValueError(f"CCAR3 requires exactly 2 views, got {self.n_views_}. Use MCCA for more than 2 views.")
        n, (p, q) = self.n_samples_, self.n_features_in_
        check_limits(p, q)
        dev = [is_device_tensor(v) for v in views_]
        if any(dev) and not all(dev):
            raise ValueError("views must be all host arrays or all CUDA tensors")
        k, eps, rho, D = int(self.latent_dimensions), float(self.eps), float(self.rho), p + q
        f32 = all(is_f32(v) for v in views_)
        h = _backend.handle_for(views_)
        # float64 copies for K1 and the fourth-moment pass, made before the handle's stream takes over
        if all(dev):
            import torch

            x64 = [v.to(torch.float64).contiguous() for v in views_]
            xptr = [int(x.data_ptr()) for x in x64]
        else:
            x64 = [h.to_device(np.ascontiguousarray(v, dtype=np.float64)) for v in views_]
            xptr = [int(b.ptr) for b in x64]
        vp = C.c_void_p

        def block(center, r0, rows, c0, cols, shift, out):
            h.check(h.lib.ccz_moments_block(h.raw, vp(mom.ptr), D, n, 1 if center else 0, r0, rows, c0, cols, float(shift),
                                            vp(out.ptr), cols))

        sp = acquire(h, views_)
        try:
            mom = h.alloc((D * D + D) * 8)
            h.moments([(xptr[0], p, p), (xptr[1], q, q)], n, _backend.F64, True, mom.ptr, pilot=False, timed=False)
            s = h.to_host(mom, (D,), offset_bytes=D * D * 8)
            if not np.all(np.isfinite(s)):
                raise ValueError("Input contains NaN or infinity.")
            mean = s / n
            center = bool(self.center)
            # Sy: the Y covariance (Ledoit-Wolf always centres; without it the products are as the views are)
            syy_d = h.alloc(q * q * 8)
            block(center, p, q, p, q, 0.0, syy_d)
            Syy = h.to_host(syy_d, (q, q))
            if self.ledoit_wolf:
                block(True, p, q, p, q, 0.0, syy_d)
                cov = Syy if center else h.to_host(syy_d, (q, q))
                mu_d = h.to_device(mean[p:])
                view = _backend.View(xptr[1], q, q)
                fourth = C.c_double(0.0)
                h.check(h.lib.ccz_rownorm4(h.raw, _backend.F64, C.byref(view), n, vp(mu_d.ptr), C.byref(fourth)))
                Sy, self.shrinkage_ = shrunk_covariance(cov.copy(), fourth.value, n)
            else:
                Sy, self.shrinkage_ = Syy, 0.0
            R_d, R = inv_sqrt_cut(h, Sy)
            # P = Sxy R
            sxy_d, P_d = h.alloc(p * q * 8), h.alloc(p * q * 8)
            block(center, 0, p, p, q, 0.0, sxy_d)
            h.gemm(False, False, p, q, q, 1.0, sxy_d.ptr, q, R_d.ptr, q, 0.0, P_d.ptr, q)
            A_d = h.alloc(p * p * 8)
            if self.highdim:
                # M = (Sxx + (rho + eps) I)^-1 = L^-T L^-1, once
                block(center, 0, p, 0, p, rho + eps, A_d)
                L_d, X_d = h.alloc(p * p * 8), h.alloc(p * p * 8)
                h.memset0(X_d.ptr, p * p * 8)
                pa, pl, px, pd = (vp * 1)(A_d.ptr), (vp * 1)(L_d.ptr), (vp * 1)(X_d.ptr), (C.c_int64 * 1)(p)
                h.check(h.lib.ccz_cholinv(h.raw, 1, pa, pd, pl, px))
                h.gemm(True, False, p, p, p, 1.0, X_d.ptr, p, X_d.ptr, p, 0.0, L_d.ptr, p)
                B, n_iter = admm(h, L_d.ptr, P_d.ptr, p, q, self.lambda_, rho, self.tol, self.max_iter)
                del X_d, L_d
            else:
                # B' = P' (Sxx + eps I)^-1 = P' L^-T L^-1
                block(center, 0, p, 0, p, eps, A_d)
                h.check(h.lib.ccz_potrf_lower(h.raw, vp(A_d.ptr), p, p))
                Pt_d = h.alloc(p * q * 8)
                h.gemm(False, True, q, p, q, 1.0, R_d.ptr, q, sxy_d.ptr, q, 0.0, Pt_d.ptr, p)
                h.check(h.lib.ccz_trsm_right_lower(h.raw, 1, q, p, vp(A_d.ptr), p, vp(Pt_d.ptr), p))
                h.check(h.lib.ccz_trsm_right_lower(h.raw, 0, q, p, vp(A_d.ptr), p, vp(Pt_d.ptr), p))
                B, n_iter = np.ascontiguousarray(h.to_host(Pt_d, (q, p)).T), 0
            if not np.all(np.isfinite(B)):
                raise np.linalg.LinAlgError("CCAR3: the coefficient matrix is not finite")
            if not np.any(B):
                U, V = np.zeros((p, k)), np.zeros((q, k))
            else:
                r = min(k, p, q)
                U0, Vt = self._svd(h, B, r)
                V0 = R @ Vt.T
                # GX = U0' Sxx U0 and Cxy = U0' Sxy V0 from the moments
                block(center, 0, p, 0, p, 0.0, A_d)
                u_d, v_d, t_d = h.to_device(U0), h.to_device(V0), h.alloc(p * r * 8)
                h.gemm(False, False, p, r, p, 1.0, A_d.ptr, p, u_d.ptr, r, 0.0, t_d.ptr, r)
                GX = U0.T @ h.to_host(t_d, (p, r))
                h.gemm(False, False, p, r, q, 1.0, sxy_d.ptr, q, v_d.ptr, r, 0.0, t_d.ptr, r)
                Cxy = U0.T @ h.to_host(t_d, (p, r))
                Wx, Wy = whiten_factor(GX, eps), whiten_factor(V0.T @ Syy @ V0, eps)
                U, V = U0 @ Wx, V0 @ Wy
                cor = np.diag(Wx.T @ Cxy @ Wy).copy()
                neg = cor < 0
                V[:, neg] *= -1.0
                cor[neg] *= -1.0
                order = np.argsort(-cor)
                U, V = U[:, order], V[:, order]
                if r < k:
                    U, V = np.hstack([U, np.zeros((p, k - r))]), np.hstack([V, np.zeros((q, k - r))])
        finally:
            release(h, sp)
        del x64
        means = [mean[:p], mean[p:]] if self.center else [np.zeros(p), np.zeros(q)]
        self._store([U, V], means, "f32" if f32 else "f64", weights_like_input=False)
        self.n_iter_ = n_iter
        return self

    @staticmethod
    def _svd(h, B, r):
        """The r leading left singular vectors of B (p x r) and right singular vectors as rows (r x q), by ``ccz_gesvj``."""
        p, q = B.shape
        if q == 1:
            return B / np.linalg.norm(B), np.ones((1, 1))
        m = min(p, q)
        b_d, u_d, s_d, vt_d = h.to_device(B), h.alloc(p * m * 8), h.alloc(m * 8), h.alloc(m * q * 8)
        h.check(h.lib.ccz_gesvj(h.raw, C.c_void_p(b_d.ptr), p, q, C.c_void_p(u_d.ptr), C.c_void_p(s_d.ptr), C.c_void_p(vt_d.ptr), None))
        return np.ascontiguousarray(h.to_host(u_d, (p, m))[:, :r]), np.ascontiguousarray(h.to_host(vt_d, (m, q))[:r])
