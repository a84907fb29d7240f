"""PLS_EY: stochastic Eckart-Young PLS, CCA_EY with ``c = 1`` (reference: ``cca_zoo/linear/gradient/_pls_ey.py:56-104``)."""

from __future__ import annotations

from cca_zoo_amd.linear.gradient._base import BaseGradientModel


class PLS_EY(BaseGradientModel):
    r"""Eckart-Young PLS: :class:`CCA_EY`'s loop with ``c = 1``, on the device.

    The initial weights are the Q factors of one standard-normal (p_i x k) draw per view (no data pass), as in the
    reference's ``random_orthonormal_weights`` (``cca_zoo/_utils/_ey.py:98-127``).  ``c`` is not a parameter
    (``"c" not in PLS_EY().get_params()``).  Deliberate differences and ``n_iter_``: see :class:`CCA_EY`.

    Args:
        latent_dimensions: Number of latent dimensions. Default is 1.
        center: Whether to subtract column means. Default True.
        learning_rate: Gradient step size. Default is 1e-2.
        max_iter: Number of gradient steps. Default is 1000.
        batch_size: Mini-batch size. ``None`` uses the full dataset.
        tol: Convergence tolerance on the objective change. Default is 1e-6.
        momentum: Momentum coefficient. Default is 0.9.
        random_state: Seed for reproducibility.
    """

    _init_kind = "pls"

    def _ridge(self) -> float:
        return 1.0
