"""Closed-form linear CCA family on the MI355X solver core."""

from cca_zoo_amd.linear._ccar3 import CCAR3
from cca_zoo_amd.linear._gcca import GCCA
from cca_zoo_amd.linear._grcca import GRCCA
from cca_zoo_amd.linear._iterative import PLS_ALS, SCCA_ADMM, SCCA_IPLS, SCCA_PMD, ElasticCCA, ParkhomenkoCCA, SCCA_Span
from cca_zoo_amd.linear._mcca import MCCA
from cca_zoo_amd.linear._partialcca import PartialCCA
from cca_zoo_amd.linear._rcca import CCA, PLS, rCCA
from cca_zoo_amd.linear._tcca import TCCA
from cca_zoo_amd.linear.gradient import CCA_EY, MCCA_EY, PLS_EY

__all__ = ["CCA", "GCCA", "GRCCA", "MCCA", "PLS", "PartialCCA", "rCCA", "CCA_EY", "PLS_EY", "MCCA_EY",
           "PLS_ALS", "SCCA_PMD", "ParkhomenkoCCA", "SCCA_Span", "SCCA_ADMM", "SCCA_IPLS", "ElasticCCA", "TCCA", "CCAR3"]
