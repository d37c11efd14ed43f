"""Optimizers with explicit gradients over the flat parameter buffer (reference ``optim/``)."""
from .flat import (FlatAdafactor, FlatAdam, FlatAdam8bit, FlatApollo, FlatGalore, FlatLAMB,
                   FlatLARS, FlatMuon, FlatSGD, make_optimizer)

__all__ = ["FlatSGD", "FlatAdam", "FlatAdam8bit", "FlatAdafactor", "FlatGalore", "FlatApollo",
           "FlatLARS", "FlatLAMB", "FlatMuon", "make_optimizer"]
