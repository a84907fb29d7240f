"""Differentiable CCA objectives on the MI355X solver core."""

from cca_zoo_amd.deep._score import score_representations
from cca_zoo_amd.deep._ssl import BarlowTwinsLoss, EYLoss, SDLLoss, VICRegLoss
from cca_zoo_amd.deep.objectives import CCALoss, GCCALoss, MCCALoss, TCCALoss

__all__ = ["CCALoss", "GCCALoss", "MCCALoss", "TCCALoss", "EYLoss", "BarlowTwinsLoss", "VICRegLoss", "SDLLoss", "score_representations"]
