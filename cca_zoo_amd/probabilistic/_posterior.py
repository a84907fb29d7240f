"""What the probabilistic models share after the fit: the posterior mean of the shared latent variable, the per-view
projections that the correlations compare, and the marginal log-likelihood by Woodbury
(``cca_zoo/probabilistic/_utils.py:11-109``, ``:167-359``).  The including class sets ``weights_``, ``means_``, ``n_views_``,
``n_features_in_``, ``n_components_`` and ``posterior_samples_`` (with a ``log_psi_{i}`` entry per view)."""

from __future__ import annotations

import ctypes as C

import numpy as np
from sklearn.utils.validation import check_is_fitted

from cca_zoo_amd._base import BaseModel, _device_project, _host_project
from cca_zoo_amd._utils._resident import MEANS_TORCH, ResidentViews
from cca_zoo_amd._utils._validation import is_device_tensor, validate_views


def align_posterior_rotation(w_samples, n_iter=3):
    """Generalised orthogonal Procrustes over posterior draws (``_utils.py:112-164``).  The model is unchanged by
    ``z -> z R``, ``W_i -> W_i R`` for any orthogonal ``R`` shared by the views, so draws of a sampler lie at different
    rotations of one subspace and their plain mean shrinks towards zero.  ``w_samples`` is ``(draws, P, k)``, the stacked
    loadings of every view.  Each pass rotates every ORIGINAL draw onto the current reference (the polar factor of
    ``draw' reference``, from its SVD), then takes the mean of the rotated draws as the next reference; the first
    reference is the plain mean.  Returns the rotated draws and the ``(draws, k, k)`` rotations of the last pass, which
    the caller applies to the same draw's ``z``.  Host NumPy: the draws are already on the host and ``k <= 32``."""
    w = np.asarray(w_samples, dtype=np.float64)
    aligned = w.copy()
    rotations = np.broadcast_to(np.eye(w.shape[2]), (w.shape[0], w.shape[2], w.shape[2])).copy()
    reference = w.mean(axis=0)
    for _ in range(int(n_iter)):
        for d in range(w.shape[0]):
            left, _, right = np.linalg.svd(w[d].T @ reference)
            rotations[d] = left @ right
            aligned[d] = w[d] @ rotations[d]
        reference = aligned.mean(axis=0)
    return aligned, rotations


class PosteriorMeanMixin:
    def _psi_inv(self):
        """Per view ``1 / max(psi_i, 1e-8)`` with ``psi_i`` the mean of the noise-variance draws, as the reference
        takes it (``_utils.py:211-214``, ``:44``)."""
        psi = [np.exp(np.array(self.posterior_samples_[f"log_psi_{i}"])).mean(axis=0) for i in range(self.n_views_)]
        return psi, [1.0 / np.maximum(ps, 1e-8) for ps in psi]

    def _information(self, views, psi_inv):
        """``sum_i (X_i - mean_i) (W_i / psi_i)`` in float64 (a CUDA tensor for CUDA views): per view one device
        projection (``BaseModel.transform``'s path), summed.  A float32 view is projected in float32, where a column of
        loadings that ARD has shrunk to 1e-146 (``drop_k=False`` keeps such columns) would flush to zero: every column is
        projected at a power-of-two scale that brings its largest loading to [0.5, 1) and scaled back in float64, which
        changes no bit of a result that was in range."""
        loadings = [w * pi[:, np.newaxis] for w, pi in zip(self.weights_, psi_inv)]
        top = np.max([np.max(np.abs(ld), axis=0) for ld in loadings], axis=0)
        scale = np.where(top > 0, 2.0 ** np.ceil(np.log2(np.where(top > 0, top, 1.0))), 1.0)
        parts = []
        for v, mu, ld in zip(views, self.means_, loadings):
            parts.append(_device_project(v, mu, ld / scale) if is_device_tensor(v) else _host_project(v, mu, ld / scale))
        if is_device_tensor(parts[0]):
            import torch

            return sum(x.double() for x in parts) * torch.as_tensor(scale, device=parts[0].device)
        return sum(np.asarray(x, dtype=np.float64) for x in parts) * scale

    def transform(self, views) -> list:
        """A one-element list: the posterior mean of the shared latent variable (``_utils.py:11-48``), float64.  Per
        view one device projection with the loadings ``W_i / psi_i``; their sum times ``Sigma_z``."""
        check_is_fitted(self)
        validated = validate_views(views, check_finite=False)
        _, psi_inv = self._psi_inv()
        precision = np.eye(self.n_components_)
        for w, pi in zip(self.weights_, psi_inv):
            precision = precision + w.T @ (w * pi[:, np.newaxis])
        sigma_z = np.linalg.inv(precision)
        info = self._information(validated, psi_inv)
        if is_device_tensor(info):
            import torch

            return [info @ torch.as_tensor(sigma_z, device=info.device)]
        if not np.all(np.isfinite(info)):
            raise ValueError("Input contains NaN or infinity.")
        return [info @ sigma_z]

    def _variates(self, views) -> list:
        """The correlations and ``score`` compare the per-view projections ``(X_i - mean_i) W_i`` (``_utils.py:217-233``)."""
        return BaseModel.transform(self, views)

    def _woodbury_log_likelihood(self, validated, psi, psi_inv, quad_diag) -> float:
        """Mean per-sample marginal log-likelihood with ``z`` integrated out (``_utils.py:51-109``) from ``quad_diag``,
        the sum over samples of ``x' Psi^-1 x``; the Woodbury correction needs the ``n x k`` projection only."""
        k, n = self.n_components_, int(validated[0].shape[0])
        m_mat = np.eye(k)
        for w, pi in zip(self.weights_, psi_inv):
            m_mat = m_mat + (w.T * pi) @ w
        log_det = sum(float(np.sum(np.log(np.maximum(ps, 1e-300)))) for ps in psi) + np.linalg.slogdet(m_mat)[1]
        proj = self._information(validated, psi_inv)
        if is_device_tensor(proj):
            proj = proj.cpu().numpy()
        quad_corr = float(np.sum((proj @ np.linalg.inv(m_mat)) * proj))
        n_features = sum(self.n_features_in_)
        return float(-0.5 * (n_features * np.log(2 * np.pi) + log_det + (quad_diag - quad_corr) / n))

    def log_likelihood(self, views) -> float:
        """Mean per-sample marginal log-likelihood with ``z`` integrated out (``_utils.py:51-109``).  The noise variance
        differs per feature, so ``x' Psi^-1 x`` is ``sum_j sum_rows fl(x - mean)^2 / psi_j`` per view (one device pass,
        ``ccz_colsumsq_weighted``) and the Woodbury correction the ``n x k`` projection; no ``n x P`` array is formed."""
        check_is_fitted(self)
        validated = validate_views(views, check_finite=False)
        psi, psi_inv = self._psi_inv()
        n = int(validated[0].shape[0])
        quad_diag = 0.0
        pd = C.POINTER(C.c_double)
        res = ResidentViews(validated, False, MEANS_TORCH)
        with res:
            h = res.handle
            dt = np.float32 if res.f32 else np.float64
            for i in range(self.n_views_):
                mu = h.to_device(np.asarray(self.means_[i], dtype=dt)) if self.center else None
                wt = np.ascontiguousarray(psi_inv[i], dtype=np.float64)
                out = C.c_double(0.0)
                h.check(h.lib.ccz_colsumsq_weighted(h.raw, res.code, C.byref(res.varr[i]), n, C.c_void_p(mu.ptr if mu else None),
                                                    wt.ctypes.data_as(pd), C.byref(out)))
                quad_diag += out.value
        return self._woodbury_log_likelihood(validated, psi, psi_inv, quad_diag)
