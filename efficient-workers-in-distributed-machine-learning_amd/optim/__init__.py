"""Optimizers with explicit gradients over the flat parameter buffer (reference ``optim/``)."""
from .flat import (FlatAdafactor, FlatAdam, FlatAdam8bit, FlatGalore, FlatLAMB, FlatLARS, FlatMuon,
                   FlatSGD, make_optimizer)

__all__ = ["FlatSGD", "FlatAdam", "FlatAdam8bit", "FlatAdafactor", "FlatGalore", "FlatLARS",
           "FlatLAMB", "FlatMuon", "make_optimizer"]
