"""Shared machinery of the kernel (dual) models: parameter resolution, kernel matrices and the fused projection.

Everything O(n^2 d) or O(n^3) runs in libccz: ``ccz_pairwise_kernel`` builds each training kernel matrix in HBM,
``ccz_kcca_solve`` / ``ccz_kgcca_solve`` solve on the device, and ``transform`` goes through ``ccz_kernel_project``,
which never writes the (n_train x n_test) kernel matrix.
"""

from __future__ import annotations

import ctypes as C

import numpy as np
from sklearn.utils.validation import check_is_fitted

from cca_zoo_amd._backend import DeviceBuffer as _DeviceBuffer
from cca_zoo_amd._base import BaseModel
from cca_zoo_amd._utils._resident import acquire, as_dtype, as_float, is_f32, release
from cca_zoo_amd._utils._validation import is_device_tensor, perview_parameter, validate_views

#: kernel names of sklearn's ``pairwise_kernels`` that the device kernels implement -> include/ccz.h CCZ_KERNEL_*
KERNEL_KINDS = {"linear": 0, "poly": 1, "polynomial": 1, "rbf": 2, "sigmoid": 3, "cosine": 4}
_USES_GAMMA = {1, 2, 3}
_KERNEL_ARGS = ("gamma", "degree", "coef0")


def kernel_specs(kernel, gamma, degree, coef0, kernel_params, n_views, n_features):
    """Per-view ``(kind, gamma, degree, coef0)`` with sklearn's ``filter_params=True`` semantics; gamma ``None`` is
    ``1 / n_features``.  Raises ``ValueError`` for a kernel the device does not implement (before any device work)."""
    kernel_ = perview_parameter("kernel", kernel, "linear", n_views)
    gamma_ = perview_parameter("gamma", gamma, None, n_views)
    degree_ = perview_parameter("degree", degree, 1.0, n_views)
    coef0_ = perview_parameter("coef0", coef0, 1.0, n_views)
    kp_ = perview_parameter("kernel_params", kernel_params, {}, n_views)
    specs = []
    for i in range(n_views):
        k = kernel_[i]
        if not isinstance(k, str) or k not in KERNEL_KINDS:
            raise ValueError(
                f"kernel {k!r} (view {i}) is not supported on the device; supported kernels: "
                f"{sorted(KERNEL_KINDS)}"
            )
        clash = set(kp_[i] or {}) & set(_KERNEL_ARGS)
        if clash:   # the reference passes gamma / degree / coef0 AND **kernel_params to pairwise_kernels
            raise TypeError(f"kernel_params repeats {sorted(clash)}, which are constructor arguments")
        kind = KERNEL_KINDS[k]
        g = gamma_[i]
        if g is None:
            g = 1.0 / n_features[i]
        specs.append((kind, float(g) if kind in _USES_GAMMA else 0.0, float(degree_[i]), float(coef0_[i])))
    return specs


class _DevView:
    """A view in HBM as libccz sees it: pointer, rows, cols, leading dimension, dtype code (owns host copies)."""

    def __init__(self, h, v):
        from cca_zoo_amd import _backend

        if is_device_tensor(v):
            if v.stride(1) != 1 or v.stride(0) < v.shape[1]:
                v = v.contiguous()
            self.keep = v
            self.ptr, self.ld = int(v.data_ptr()), int(v.stride(0))
            self.dtype = _backend.F32 if v.element_size() == 4 else _backend.F64
        else:
            v = np.ascontiguousarray(v)
            self.keep = h.to_device(v)
            self.ptr, self.ld = int(self.keep.ptr), int(v.shape[1])
            self.dtype = _backend.F32 if v.dtype == np.float32 else _backend.F64
        self.n, self.d = int(v.shape[0]), int(v.shape[1])


def pairwise_kernel(h, A, B, spec, K_ptr, ldk, meanA=None, meanB=None):
    """K (device float64) = kernel(A - meanA, B - meanB); A, B are ``_DevView`` (same dtype); B is A: symmetric."""
    kind, g, deg, c0 = spec
    if A.dtype != B.dtype:
        raise ValueError("both sides of a kernel matrix must have the same dtype")
    h.check(h.lib.ccz_pairwise_kernel(h.raw, A.dtype, C.c_void_p(A.ptr), A.n, A.ld, _vp(meanA), C.c_void_p(B.ptr), B.n,
                                      B.ld, _vp(meanB), A.d, kind, g, deg, c0, C.c_void_p(int(K_ptr)), int(ldk)))


def kernel_project(h, A, B, spec, W_ptr, k, out_ptr, ldo, meanA=None, meanB=None):
    """out (B.n x k, device float64) = kernel(A - meanA, B - meanB)' W without forming the kernel matrix."""
    kind, g, deg, c0 = spec
    if A.dtype != B.dtype:
        raise ValueError("both sides of a kernel matrix must have the same dtype")
    h.check(h.lib.ccz_kernel_project(h.raw, A.dtype, C.c_void_p(A.ptr), A.n, A.ld, _vp(meanA), C.c_void_p(B.ptr), B.n,
                                     B.ld, _vp(meanB), A.d, kind, g, deg, c0, C.c_void_p(int(W_ptr)), int(k), int(k),
                                     C.c_void_p(int(out_ptr)), int(ldo)))


def _vp(x):
    return None if x is None else C.c_void_p(int(x))


class KernelModel(BaseModel):
    """Common surface of :class:`KCCA` and :class:`KGCCA`: validation, kernel matrices on the device, transform through
    the fused projection, loadings from one K1 pass.  Subclasses implement ``_solve``."""

    def _solve(self, h, K_ptrs, n, k):  # pragma: no cover - abstract
        raise NotImplementedError

    def _kernel_args(self):
        return self.kernel, self.gamma, self.degree, self.coef0, self.kernel_params

    def fit(self, views, y=None):
        from cca_zoo_amd import _backend, _dist

        if _dist.is_sharded():
            raise NotImplementedError(
                f"{type(self).__name__} solves an (n x n) dual problem, which does not shard by rows: "
                "fit it outside row_sharded()"
            )
        self._validate_params()
        validated = [as_float(v) for v in validate_views(views, check_finite=False)]
        m = len(validated)
        n = int(validated[0].shape[0])
        n_features = [int(v.shape[1]) for v in validated]
        specs = kernel_specs(*self._kernel_args(), m, n_features)
        k = int(self.latent_dimensions)
        if k > n:
            raise ValueError(f"latent_dimensions={k} exceeds the number of samples ({n})")
        if n < 2:
            raise ValueError("at least 2 samples are required")
        self._check_limits(m, n)
        dev = [is_device_tensor(v) for v in validated]
        if any(dev) and not all(dev):
            raise ValueError("views must be all host arrays or all CUDA tensors")
        # the reference's _setup_fit: means in the input dtype, centred training views kept for transform
        if all(dev):
            self.means_ = [v.mean(dim=0) if self.center else v.new_zeros(v.shape[1], dtype=v.dtype) for v in validated]
            self.train_views_ = [v - mu for v, mu in zip(validated, self.means_)] if self.center else list(validated)
            self.means_ = [mu.detach().cpu().numpy() for mu in self.means_]
        else:
            if self.center:
                self.means_ = [v.mean(axis=0) for v in validated]
                self.train_views_ = [v - mu for v, mu in zip(validated, self.means_)]
            else:
                self.means_ = [np.zeros(p) for p in n_features]
                self.train_views_ = list(validated)
            if not all(np.all(np.isfinite(v)) for v in self.train_views_):
                raise ValueError("Input contains NaN or infinity.")
        self.n_views_, self.n_features_in_, self.n_samples_ = m, n_features, n
        self._specs = specs

        h = _backend.handle_for(validated)
        # every conversion (contiguous copies, host -> device) is enqueued BEFORE the handle's stream takes over, and
        # every tensor it reads stays referenced until the caller's stream has been made to wait for it again
        dviews = [_DevView(h, v) for v in self.train_views_]
        sp = acquire(h, validated)
        try:
            Ks = [h.alloc(n * n * 8) for _ in range(m)]
            for i, A in enumerate(dviews):
                pairwise_kernel(h, A, A, specs[i], Ks[i].ptr, n)
            W, vals, kk = self._solve(h, [K.ptr for K in Ks], n, k)
        finally:
            release(h, sp)
        self.weights_ = [w.copy() for w in W]
        self.eigenvalues_ = vals
        del Ks, dviews
        return self

    def _check_limits(self, m, n):
        pass

    def transform(self, views) -> list:
        """``kernel(train_views_[i], views[i])' @ weights_[i]`` per view through ``ccz_kernel_project`` (the kernel
        matrix is never formed).  Deliberate parity with the reference (``_kcca.py:134-146``): the kernel is taken
        between the CENTRED training views and the test views AS GIVEN -- the test views are not centred.  Host arrays
        in: float64 arrays out (whatever the input dtype, as the reference's float64 weights make them).  CUDA tensors
        in: float64 CUDA tensors out."""
        from cca_zoo_amd import _backend

        check_is_fitted(self)
        validated = [as_float(v) for v in validate_views(views, check_finite=False)]
        if len(validated) != self.n_views_:
            raise ValueError(f"expected {self.n_views_} views, got {len(validated)}")
        h = _backend.handle_for(validated)
        # stage 1, on the caller's stream: the training view on the test view's side (device / host), both sides in one
        # dtype (float32 only when both are float32, as sklearn's check_pairwise_arrays does; else float64), contiguous
        prepared = []
        for i, v in enumerate(validated):
            if int(v.shape[1]) != self.n_features_in_[i]:
                raise ValueError(f"view {i} has {v.shape[1]} features, the model was fitted on {self.n_features_in_[i]}")
            tr = self.train_views_[i]
            if is_device_tensor(v):
                import torch

                if not is_device_tensor(tr):
                    tr = torch.as_tensor(np.ascontiguousarray(tr), device=v.device)
                elif tr.device != v.device:
                    tr = tr.to(v.device)
            elif is_device_tensor(tr):
                tr = tr.detach().cpu().numpy()
            if not (is_f32(tr) and is_f32(v)):
                tr, v = as_dtype(tr, _backend.F64), as_dtype(v, _backend.F64)
            A, B = _DevView(h, tr), _DevView(h, v)
            k = int(self.weights_[i].shape[1])
            if is_device_tensor(v):
                import torch

                z = torch.empty((B.n, k), dtype=torch.float64, device=v.device)
                zp = z.data_ptr()
            else:
                z = h.alloc(max(B.n * k * 8, 8))
                zp = z.ptr
            prepared.append((A, B, k, z, zp))
        # stage 2, on the handle's stream; the caller's stream waits for it before anything above is released
        sp = acquire(h, validated)
        try:
            keep = []
            for i, (A, B, k, z, zp) in enumerate(prepared):
                wd = h.to_device(np.ascontiguousarray(self.weights_[i], dtype=np.float64))
                keep.append(wd)
                kernel_project(h, A, B, self._specs[i], wd.ptr, k, zp, k)
        finally:
            release(h, sp)
        out = []
        for A, B, k, z, zp in prepared:
            if isinstance(z, _DeviceBuffer):
                z = h.to_host(z, (B.n, k))
                if not np.all(np.isfinite(z)):
                    raise ValueError("Input contains NaN or infinity.")
            out.append(z)
        del prepared, keep
        return out

    def get_factor_loadings(self, views) -> list:
        """Pearson correlation of every input feature with every canonical variate of its view (the reference's generic
        formula over ``transform``, ``_base.py:208-234``).  The weights are dual (n x k), so the variates come from
        ``transform`` and each view takes ONE K1 pass over ``[X_i | Z_i]``; ``ccz_factor_loadings`` with the selector
        ``W = [0; I_k]`` then reads ``corr(x_j, z_t)`` off those moments on the device."""
        from cca_zoo_amd import _backend
        from cca_zoo_amd._moments import compute_moments

        check_is_fitted(self)
        validated = [as_float(v) for v in validate_views(views, check_finite=False)]
        zs = self.transform(validated)
        out = []
        for v, z in zip(validated, zs):
            h = _backend.handle_for([v])
            if is_device_tensor(v):
                x = v.to(z.dtype)
                mom, keep, n, dims, _ = compute_moments([x, z], h)
            else:
                mom, keep, n, dims, _ = compute_moments([np.asarray(v, dtype=np.float64), z], h)
            d, k = int(dims[0]), int(dims[1])
            D = d + k
            h.moments_symmetrize(mom, D)
            sel = np.zeros((D, k))
            sel[d:, :] = np.eye(k)
            wd = h.to_device(sel)
            od = h.alloc(D * k * 8)
            h.check(h.lib.ccz_factor_loadings(h.raw, C.c_void_p(int(mom)), int(n), D, C.c_void_p(wd.ptr), k,
                                              C.c_void_p(od.ptr)))
            out.append(h.to_host(od, (D, k))[:d].copy())
            del keep
        return out
