"""MCCA_EY: multiview Eckart-Young CCA (reference: ``cca_zoo/linear/gradient/_mcca_ey.py:46-61``)."""

from __future__ import annotations

from cca_zoo_amd.linear.gradient._cca_ey import CCA_EY


class MCCA_EY(CCA_EY):
    """Eckart-Young CCA for two or more views: the same loss, loop and device path as :class:`CCA_EY`, whose
    launches already take every view at once (one launch per stage for any number of views, at most 16)."""
