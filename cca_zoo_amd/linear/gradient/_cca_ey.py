"""CCA_EY: Eckart-Young CCA, ridge-blended with PLS_EY (reference: ``cca_zoo/linear/gradient/_cca_ey.py:134-225``)."""

from __future__ import annotations

from numbers import Real
from typing import Any, ClassVar

from sklearn.utils._param_validation import Interval

from cca_zoo_amd.linear.gradient._base import BaseGradientModel


class CCA_EY(BaseGradientModel):
    r"""Eckart-Young CCA by mini-batch momentum gradient descent, every step on the device.

    Minimises $-2\operatorname{tr}(C - cV) + \operatorname{tr}(V_c V_c)$ with $V_c = (1 - c)V + cB$ over the
    embeddings $Z_i = X_i W_i$: $C$ and $V$ are the mean pairwise and mean auto-covariances of the embeddings of a
    mini-batch, $B = \frac{1}{M}\sum_i W_i^\top W_i$.  ``c = 0`` is plain CCA_EY, ``c = 1`` is PLS_EY's loss.  The
    steps, the initialisation (``z0`` of one mini-batch projected on the device, ``R`` from the host's
    ``np.linalg.qr``) and the RNG draw order follow the reference, so fits follow its trajectory, not only its fixed
    point.  As in the reference, ``c = 0`` can diverge when a batch has few rows for its width; the weights are then
    non-finite and no error is raised.

    Differences from the reference, on purpose:

    - ``latent_dimensions`` larger than the narrowest view raises ``ValueError`` (the reference fails later with a
      shape error); at most 128 latent dimensions.
    - ``fit`` inside :func:`cca_zoo_amd.row_sharded` raises ``NotImplementedError``.
    - With a full batch (``batch_size=None`` or ``>= n_samples``) the per-step row permutation only changes the order
      of summation, so the device uses the rows in order and the host draws nothing inside the loop.  The
      permutation of the initialisation is drawn and used (the Householder ``R`` depends on the row order).
    - float32 views: the two products per step run on the fp32 matrix pipe (centred fp32 rows times weights rounded
      to fp32, reduced in fp64); the weights, the velocity and all k x k algebra stay float64.  The reference
      upcasts every batch to float64.  float64 views: float64 throughout.

    Attributes (beyond the reference's): ``n_iter_``, the number of gradient steps applied -- ``max_iter``, or the
    step whose objective change fell below ``tol``.

    Args:
        latent_dimensions: Number of latent dimensions. Default is 1.
        center: Whether to subtract column means. Default True.
        c: Ridge blend in ``[0, 1]`` between CCA_EY (0) and PLS_EY (1). Default is 0.
        learning_rate: Gradient step size. Default is 1e-2.
        max_iter: Number of gradient steps. Default is 1000.
        batch_size: Mini-batch size. ``None`` uses the full dataset.
        tol: Convergence tolerance on the objective change between consecutive steps. Default is 1e-6.
        momentum: Momentum coefficient. Default is 0.9.
        random_state: Seed of the one ``np.random.default_rng`` that draws the initial weights and the batches.
    """

    _parameter_constraints: ClassVar[dict[str, list[Any]]] = {
        **BaseGradientModel._parameter_constraints,
        "c": [Interval(Real, 0, 1, closed="both")],
    }

    def __init__(
        self,
        latent_dimensions: int = 1,
        center: bool = True,
        c: float = 0.0,
        learning_rate: float = 1e-2,
        max_iter: int = 1000,
        batch_size: int | None = None,
        tol: float = 1e-6,
        momentum: float = 0.9,
        random_state: int | None = None,
    ) -> None:
        super().__init__(
            latent_dimensions=latent_dimensions,
            center=center,
            learning_rate=learning_rate,
            max_iter=max_iter,
            batch_size=batch_size,
            tol=tol,
            momentum=momentum,
            random_state=random_state,
        )
        self.c = c
