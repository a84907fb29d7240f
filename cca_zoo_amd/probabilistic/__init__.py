"""Probabilistic models on the MI355X solver core: GFA (group factor analysis), every VB iteration on the device."""

from cca_zoo_amd.probabilistic._gfa import GFA

__all__ = ["GFA"]
