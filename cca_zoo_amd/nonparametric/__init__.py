"""Nonparametric (kernel) CCA on the MI355X solver core: kernel matrices, solve and projection in libccz."""

from cca_zoo_amd.nonparametric._kcca import KCCA
from cca_zoo_amd.nonparametric._kgcca import KGCCA
from cca_zoo_amd.nonparametric._ktcca import KTCCA

__all__ = ["KCCA", "KGCCA", "KTCCA"]
