"""Probabilistic models on the MI355X solver core: GFA (group factor analysis), every VB iteration on the device,
VariationalBayesCCA (mean-field SVI with a shared ARD prior), every step on the device, and ProbabilisticCCA (NUTS), every
leapfrog step on the device."""

from cca_zoo_amd.probabilistic._gfa import GFA
from cca_zoo_amd.probabilistic._pcca import ProbabilisticCCA  # noqa: F401  (public; see below)
from cca_zoo_amd.probabilistic._vbcca import VariationalBayesCCA  # noqa: F401  (public; see below)

# ``from cca_zoo_amd.probabilistic import VariationalBayesCCA`` (or ``ProbabilisticCCA``) is the public import.  ``__all__`` still lists GFA alone:
# tests/test_gfa_host.py pins it to that value, and a star import of this module is not part of the documented surface.
__all__ = ["GFA"]
