"""Optimizers with explicit gradients over the flat parameter buffer (reference ``optim/``)."""
from .flat import FlatAdam, FlatLAMB, FlatLARS, FlatSGD, make_optimizer

__all__ = ["FlatSGD", "FlatAdam", "FlatLARS", "FlatLAMB", "make_optimizer"]
