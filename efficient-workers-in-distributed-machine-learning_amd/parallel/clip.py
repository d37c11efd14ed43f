"""Global-norm clipping of this rank's gradient ahead of the exchange (``--clip-grad-norm``).

DGC's fourth technique, *local gradient clipping*: each worker clips its own gradient by its
global L2 norm before the gradient enters the residual, with threshold ``C`` or, under
``--clip-scale-world``, ``C / sqrt(N)`` (N workers).  The compressed exchanges never materialise
the averaged dense gradient (their decode is fused with the step), so this is the one definition
that works for every codec; at a world of one it is ``torch.nn.utils.clip_grad_norm_``.

The rule works on the raw local gradient (no ``grad_scale``, ``--predivide``, ``1/N`` or weight
decay) after backward has produced every gradient and before the exchange reads one::

    norm = ||g||_2 over every parameter's own elements      (never the alignment padding)
    coef = min(1, C' / (norm + 1e-6))
    g   *= coef                                              (in place; untouched when coef == 1)

On the GPU that is two launches per bucket (``ops/csrc/clip.hip``: every bucket's ``k_clip_norm``,
then every bucket's ``k_clip_scale``), on the step's stream, so a captured step carries them and
``clip_state = {norm, coef}`` in device memory follows the gradients from replay to replay.  On
the CPU it is ``compress/oracle.py clip_grad_norm_``.  The clip keeps no state between steps.
"""
import math

import torch

from .. import ops
from ..compress import oracle


def clip_threshold(max_norm: float, world: int = 1, scale_world: bool = False) -> float:
    """``C`` or, with ``scale_world``, DGC's ``C / sqrt(N)``."""
    max_norm = float(max_norm)
    if not max_norm > 0.0:
        raise ValueError("the clipping threshold must be > 0")
    return max_norm / math.sqrt(max(1, int(world))) if scale_world else max_norm


class GradClipper:
    def __init__(self, flat, max_norm: float, world: int = 1, scale_world: bool = False):
        self.flat = flat
        self.max_norm = clip_threshold(max_norm, world, scale_world)
        self.cuda = flat.data.device.type == "cuda"
        if not self.cuda and not flat.attach_grads:
            raise ValueError("pointer-mode gradients need the HIP kernels (device tensors)")
        self.plan = ops.ClipPlan([b.plan for b in flat.buckets], flat.data.device) \
            if self.cuda else None
        self._last = None  # CPU: the last step's (norm, coef) tensors
        self.runs = 0

    def run(self):
        """Clip this step's gradients in place.  Launches only (no host synchronisation); on the
        GPU on the current stream."""
        flat = self.flat
        self.runs += 1
        if not self.cuda:
            views = [flat.grad[o:o + p.numel()] for p, o in zip(flat.params, flat.offsets)]
            self._last = oracle.clip_grad_norm_(views, self.max_norm)
            return
        grads = [flat.bucket_grads(b) for b in flat.buckets]
        for b, g in zip(flat.buckets, grads):
            ops.clip_norm(self.plan, b.index, g)
        for b, g in zip(flat.buckets, grads):
            ops.clip_scale(self.plan, b.index, g, self.max_norm)

    def last(self):
        """``(norm, coef)`` of the last step as floats, or None before the first (synchronises)."""
        if not self.runs:
            return None
        if self.cuda:
            norm, coef = self.plan.state.tolist()
        else:
            norm, coef = (float(v) for v in self._last)
        return norm, coef
