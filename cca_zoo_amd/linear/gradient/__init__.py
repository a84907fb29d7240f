"""Gradient-descent (Eckart-Young) CCA models for views too wide for the Gram route.

Reference: ``cca_zoo/linear/gradient``.  The models never form a p x p matrix: each step reads a mini-batch of rows
and does two skinny products per view on the device (``csrc/ey.hip``).
"""

from cca_zoo_amd.linear.gradient._cca_ey import CCA_EY
from cca_zoo_amd.linear.gradient._mcca_ey import MCCA_EY
from cca_zoo_amd.linear.gradient._pls_ey import PLS_EY

__all__ = ["PLS_EY", "CCA_EY", "MCCA_EY"]
