"""KCCA -- kernel canonical correlation analysis with the kernel matrices and the solve on the device.

Reference: cca_zoo/nonparametric/_kcca.py.  ``fit`` builds each view's n x n kernel matrix with ``ccz_pairwise_kernel``
(fp64 matrix pipe, only the upper triangle computed) and solves the reference's generalised eigenproblem

    A v = lambda B v,   v'Bv = 1,   A = (cov(hstack K) - blockdiag cov(K_i)) / M,
    B = (blockdiag(c_i K_i + (1 - c_i) K_i^2) + shift I) / M,   shift = max(0, eps - lambda_min(blockdiag))

with ``ccz_kcca_solve``: one eigendecomposition per kernel matrix turns B into a diagonal scaling, after which two
views are a top-k SVD of the whitened cross-covariance and more views a dense EVD of the whitened A.
"""

from __future__ import annotations

import ctypes as C

import numpy as np

from cca_zoo_amd._utils._validation import perview_parameter
from cca_zoo_amd.nonparametric._kernel_base import KernelModel


class KCCA(KernelModel):
    """Kernel CCA (Hardoon, Szedmak & Shawe-Taylor, 2004).

    Args:
        latent_dimensions: number of latent dimensions (default 1).
        center: subtract column means before fitting (default True).
        c: regularisation parameter(s) (default 0.1); scalar or one per view.
        kernel: ``"linear"``, ``"poly"`` / ``"polynomial"``, ``"rbf"``, ``"sigmoid"`` or ``"cosine"``, or one per view.
        gamma: kernel gamma(s); ``None`` is ``1 / n_features`` (scikit-learn's default).
        degree: polynomial degree(s) (default 1.0; a real exponent).
        coef0: coef0 of the polynomial / sigmoid kernels (default 1.0).
        kernel_params: extra per-view keyword arguments (ignored by the supported kernels, as with ``filter_params``).
        eps: floor of the smallest eigenvalue of B (default 1e-3).

    ``weights_`` are the dual coefficients (n_samples x latent_dimensions per view); ``eigenvalues_`` the top-k
    generalised eigenvalues.
    """

    def __init__(self, latent_dimensions: int = 1, center: bool = True, c=0.1, kernel="linear", gamma=None,
                 degree=1.0, coef0=1.0, kernel_params=None, eps: float = 1e-3) -> None:
        super().__init__(latent_dimensions=latent_dimensions, center=center)
        self.c = c
        self.kernel = kernel
        self.gamma = gamma
        self.degree = degree
        self.coef0 = coef0
        self.kernel_params = kernel_params
        self.eps = eps

    def _check_limits(self, m, n):
        if m > 2 and m * n > 16384:
            raise ValueError(f"KCCA with {m} views solves a dense eigenproblem of size n_views * n_samples = {m * n}; "
                             "the limit is 16384")

    def _solve(self, h, K_ptrs, n, k):
        m = len(K_ptrs)
        c_ = [float(v) for v in perview_parameter("c", self.c, 0.1, m)]
        Wd = h.alloc(m * n * k * 8)
        vals = np.zeros(k)
        kout = C.c_int(0)
        ka = (C.c_void_p * m)(*K_ptrs)
        ca = (C.c_double * m)(*c_)
        h.check(h.lib.ccz_kcca_solve(h.raw, ka, m, n, ca, float(self.eps), k, C.c_void_p(Wd.ptr),
                                     vals.ctypes.data_as(C.POINTER(C.c_double)), C.byref(kout)))
        kk = kout.value
        W = h.to_host(Wd, (m, n, kk))
        return [W[i] for i in range(m)], vals[:kk], kk
