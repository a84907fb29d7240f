"""What the probabilistic models share after the fit: the posterior mean of the shared latent variable, the per-view
projections that the correlations compare, and the marginal log-likelihood by Woodbury
(``cca_zoo/probabilistic/_utils.py:11-109``, ``:167-359``).  The including class sets ``weights_``, ``means_``, ``n_views_``,
``n_features_in_``, ``n_components_`` and ``posterior_samples_`` (with a ``log_psi_{i}`` entry per view)."""

from __future__ import annotations

import numpy as np
from sklearn.utils.validation import check_is_fitted

from cca_zoo_amd._base import BaseModel, _device_project, _host_project
from cca_zoo_amd._utils._validation import is_device_tensor, validate_views


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
