"""KGCCA -- kernel generalised CCA with the kernel matrices and the solve on the device.

Reference: cca_zoo/nonparametric/_kgcca.py.  ``fit`` builds each view's kernel matrix with ``ccz_pairwise_kernel`` and
``ccz_kgcca_solve`` forms

    Q = sum_i mu_i K_i B_i^-1 K_i,   B_i = c_i K_i + (1 - c_i) K_i^2 + shift_i I,

takes its top-k eigenvectors T and returns ``weights_i = pinv(K_i) T`` (NumPy's cutoff), all through one
eigendecomposition per kernel matrix.  ``view_weights`` must be non-negative (Q is then positive semi-definite and its
top-k eigenvectors are the top-k left singular vectors of a factor of it).
"""

from __future__ import annotations

import ctypes as C

import numpy as np

from cca_zoo_amd._utils._validation import perview_parameter
from cca_zoo_amd.nonparametric._kernel_base import KernelModel


class KGCCA(KernelModel):
    """Kernel generalised CCA (Tenenhaus, Philippe & Frouin, 2015).

    Args:
        latent_dimensions: number of latent dimensions (default 1).
        center: subtract column means before fitting (default True).
        c: regularisation parameter(s) (default 0.1).
        kernel, gamma, degree, coef0, kernel_params: as in :class:`KCCA`.
        view_weights: non-negative per-view weights mu_i (default: all 1).
        eps: floor of each B_i's smallest eigenvalue (default 1e-6).

    ``weights_`` are the dual coefficients (n_samples x latent_dimensions per view); ``eigenvalues_`` the top-k
    eigenvalues of Q.
    """

    def __init__(self, latent_dimensions: int = 1, center: bool = True, c=0.1, kernel="linear", gamma=None,
                 degree=1.0, coef0=1.0, kernel_params=None, view_weights=None, eps: float = 1e-6) -> None:
        super().__init__(latent_dimensions=latent_dimensions, center=center)
        self.c = c
        self.kernel = kernel
        self.gamma = gamma
        self.degree = degree
        self.coef0 = coef0
        self.kernel_params = kernel_params
        self.view_weights = view_weights
        self.eps = eps

    def _check_limits(self, m, n):
        mu = [float(v) for v in perview_parameter("view_weights", self.view_weights, 1.0, m)]
        if any(not (v >= 0.0) for v in mu):
            raise ValueError(f"view_weights must be non-negative, got {mu}")

    def _solve(self, h, K_ptrs, n, k):
        m = len(K_ptrs)
        c_ = [float(v) for v in perview_parameter("c", self.c, 0.1, m)]
        mu = [float(v) for v in perview_parameter("view_weights", self.view_weights, 1.0, m)]
        Wd = h.alloc(m * n * k * 8)
        vals = np.zeros(k)
        kout = C.c_int(0)
        ka = (C.c_void_p * m)(*K_ptrs)
        h.check(h.lib.ccz_kgcca_solve(h.raw, ka, m, n, (C.c_double * m)(*c_), (C.c_double * m)(*mu), float(self.eps), k,
                                      C.c_void_p(Wd.ptr), vals.ctypes.data_as(C.POINTER(C.c_double)), C.byref(kout)))
        kk = kout.value
        W = h.to_host(Wd, (m, n, kk))
        return [W[i] for i in range(m)], vals[:kk], kk
