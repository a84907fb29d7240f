"""Tree-based multiview models: :class:`TreeCCA` (boosted-tree CCA, histogram tree growth on the device)."""

from cca_zoo_amd.tree._treecca import TreeBooster, TreeCCA

__all__ = ["TreeBooster", "TreeCCA"]
