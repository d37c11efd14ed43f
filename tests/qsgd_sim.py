"""Inputs and the unbiasedness statistic shared by the dense QSGD tests: the oracle's on the CPU
(tests/unit/test_compress.py) and the kernels' on the device (tests/kernels/test_qsgd_codec_hip.py)
see the same buckets, so a figure measured on one side holds for the other."""
import math

import torch

from ewdml.compress.plan import BucketPlan
from ewdml.compress.rng import stream_key

BUCKET_OFFSET = 4096 + 192  # non-zero: it enters the RNG index
UNBIASED = (8192 + 13, 10, 5000, 1, 64)
UNBIASED_SEED = 5
UNBIASED_KEYS = [stream_key(7, s, 0) for s in range(64)]
UNBIASED_Z = 6.0


def make_plan(numels, bucket_offset=BUCKET_OFFSET):
    """Tensors packed at multiples of 64 elements, as parallel/flat.py lays them out."""
    offs, o = [], 0
    for n in numels:
        offs.append(o)
        o += (n + 63) // 64 * 64
    return BucketPlan(list(numels), offs, 1.0, bucket_offset, o)


def bucket(plan, seed, gap=0.0):
    """Random tensors of differing magnitudes (sigma 0.05 .. 0.25), ``gap`` between them."""
    gen = torch.Generator().manual_seed(seed)
    x = torch.full((plan.length,), gap)
    for off, n in zip(plan.offsets, plan.numels):
        x[off:off + n] = torch.randn(n, generator=gen) * (0.05 + 0.2 * float(
            torch.rand(1, generator=gen)))
    return x


def worst_z(plan, g, mean, levels):
    """The largest |mean - x| over every element, in units of step / (2 sqrt(K)) with step =
    |x|_2 / levels: a decoded element is step * (floor + Bernoulli(frac)), so that unit bounds the
    standard deviation of the mean of K independent roundings.  ``mean``: float64."""
    worst = 0.0
    for off, n in zip(plan.offsets, plan.numels):
        x = g[off:off + n].double()
        unit = float(x.norm()) / levels / (2 * math.sqrt(len(UNBIASED_KEYS)))
        worst = max(worst, float((mean[off:off + n] - x).abs().max()) / unit)
    return worst
