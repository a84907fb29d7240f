"""KTCCA -- kernel tensor CCA: kernel matrices, whitening, cross-moment tensor and CP-ALS on the device.

Reference: ``cca_zoo/nonparametric/_ktcca.py``.  ``fit`` builds each view's n x n kernel matrix with
``ccz_pairwise_kernel``, forms ``cov_i = (1 - c_i) K_i K_i + c_i K_i`` with the float64 GEMM, takes its inverse square root
as :class:`cca_zoo_amd.linear.TCCA` does (same ``eps`` shift, device Jacobi EVD), whitens ``H_i = K_i cov_i^-1/2`` and
decomposes the cross-moment tensor of the ``H_i`` (``ccz_kr_moment``, then ``csrc/cp_als.hip``).  The tensor has ``n^V``
entries, so ``n^V <= 2^24``: 256 samples for three views.  ``transform`` is the kernel models' fused projection
(``ccz_kernel_project``) and keeps the reference's asymmetry: the training views are stored centred, test rows are used
as given.  The factor step is the CP-ALS stated in ``include/ccz.h``, not tensorly's code (see ``linear/_tcca.py``).
"""

from __future__ import annotations

import numpy as np

from cca_zoo_amd._utils._validation import perview_parameter
from cca_zoo_amd.linear._tcca import check_tensor_limits, decompose, inv_sqrt_shifted
from cca_zoo_amd.nonparametric._kernel_base import KernelModel


class KTCCA(KernelModel):
    """Kernel tensor CCA (Kim, Wong & Cipolla 2007).

    Args:
        latent_dimensions: number of latent dimensions (default 1).
        center: subtract column means before fitting (default True).
        c: regularisation parameter(s) (default 0.1); scalar or one per view.
        kernel: ``"linear"``, ``"poly"`` / ``"polynomial"``, ``"rbf"``, ``"sigmoid"`` or ``"cosine"``, or one per view.
        gamma: kernel gamma(s); ``None`` is ``1 / n_features`` (scikit-learn's default).
        degree: polynomial degree(s) (default 1.0; a real exponent).
        coef0: coef0 of the polynomial / sigmoid kernels (default 1.0).
        kernel_params: extra per-view keyword arguments (ignored by the supported kernels, as with ``filter_params``).
        eps: floor of the smallest eigenvalue of every ``cov_i`` (default 1e-3).
        random_state: accepted for compatibility; unused (the decomposition is deterministic).

    ``weights_`` are the dual coefficients (n_samples x latent_dimensions per view).  Not in the reference: ``n_iter_``
    and ``rec_error_`` (CP-ALS iterations and the relative reconstruction error after each).

    Differences from the reference, on purpose: 2 to 8 views, ``n_samples ** n_views <= 2^24``, ``latent_dimensions <=
    min(32, n_samples)``, no ``row_sharded()`` fits, unsupported kernels and ``kernel_params`` clashes as in
    :class:`KCCA`, and the decomposition is the written-out CP-ALS.
    """

    def __init__(self, latent_dimensions: int = 1, center: bool = True, c=0.1, kernel="linear", gamma=None, degree=1.0,
                 coef0=1.0, kernel_params=None, eps: float = 1e-3, random_state=None) -> None:
        super().__init__(latent_dimensions=latent_dimensions, center=center)
        self.c = c
        self.kernel = kernel
        self.gamma = gamma
        self.degree = degree
        self.coef0 = coef0
        self.kernel_params = kernel_params
        self.eps = eps
        self.random_state = random_state

    def _check_limits(self, m, n):
        perview_parameter("c", self.c, 0.1, m)
        check_tensor_limits("KTCCA", int(self.latent_dimensions), [n] * m)

    def _solve(self, h, K_ptrs, n, k):
        m = len(K_ptrs)
        c_ = [float(v) for v in perview_parameter("c", self.c, 0.1, m)]
        F_host, H, keep = [], [], []
        for Kp, ci in zip(K_ptrs, c_):
            KK = h.alloc(n * n * 8)
            h.gemm(False, False, n, n, n, 1.0, Kp, n, Kp, n, 0.0, KK.ptr, n)
            cov = (1.0 - ci) * h.to_host(KK, (n, n)) + ci * h.to_host(Kp, (n, n))
            Fd, Fh = inv_sqrt_shifted(h, 0.5 * (cov + cov.T), float(self.eps))
            Hd = h.alloc(n * n * 8)
            h.gemm(False, False, n, n, n, 1.0, Kp, n, Fd.ptr, n, 0.0, Hd.ptr, n)
            F_host.append(Fh), H.append(Hd), keep.append(Fd)
        factors, trace = decompose(h, [b.ptr for b in H], [n] * m, n, k)
        self.n_iter_ = int(trace.size)
        self.rec_error_ = trace
        return [f @ a for f, a in zip(F_host, factors)], None, k

    def fit(self, views, y=None):
        super().fit(views, y)
        del self.eigenvalues_       # the kernel base's slot for a spectrum; this model has none
        return self
