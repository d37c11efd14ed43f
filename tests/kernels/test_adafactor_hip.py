"""Adafactor's kernels (ops/csrc/adafactor.hip) through ``FlatAdafactor.step_range`` on the GPU,
against ``compress/oracle.py adafactor_apply`` in float64.  One step (the 7th) from a preloaded
positive state over a flat buffer of one matrix and one vector, ``grad_scale = 0.5``.

Update: with D a tensor's update (new - old), ``|D_hip - D_64| <= 3 |D_oracle32 - D_64|`` in norm,
the oracle's own fp32 error being the yardstick (floor ``2^-23 |D_64|`` where it is 0).

R and C: ``|x_hip - x_64| <= (L + c) 2^-24 x_64`` per entry, L = ``ops.ADAFACTOR_SUM_CHAIN``.  A
statistic is ``x b2 + (1 - b2) mean(q)`` of non-negative terms, so relative errors add at first
order: L roundings at the most from a gradient to its tile's partial (the sums over tiles are
fp64), and c = 4 for the mean (the fp64 total divided and rounded once), the two multiplies and
the add.  L counts every fp32 addition of the chain, the first one into a zero accumulator
included; that one is exact, so the L roundings are the term's own ``g * g`` and the L - 1
additions that do round.  ``+ 1e-30`` returns ``g * g`` unchanged, a relative 1e-30 / g^2 away
from the exact q (under 2^-60 for |g| > 2e-6; smaller terms do not weigh in the sum), and with a
zero gradient q is the fp32 constant, one rounding from 1e-30.  The ratios are printed.

A vector's v is element-wise with no sum: bitwise the fp32 oracle's."""
import functools

import pytest
import torch

from ewdml import ops
from ewdml.compress import oracle
from ewdml.optim import FlatAdafactor
from tests.layerwise_ref import make_flat, make_grad

pytestmark = pytest.mark.gpu

KW = dict(lr=1e-2, weight_decay=1e-2)
# under one tile, unaligned | LeNet conv1, unaligned | one past the tile both ways, aligned |
# LeNet fc1: many bands and strips, both ragged | one partial band, 18 strips | many bands, m < 8,
# unaligned | a single row | zero gradient
SHAPES = [(3, 7), (20, 25), (33, 260), (500, 800), (10, 4608), (1030, 6), (1, 8193), "zero"]
F32, BF16 = torch.float32, torch.bfloat16
CASES = [(s, F32, ()) for s in SHAPES] + [((33, 260), BF16, ()), ((500, 800), BF16, ())] + [
    ((500, 800), F32, o) for o in ((("clip", 0.1),), (("clip", 1e9),), (("beta1", 0.9),),
                                   (("scale_parameter", True),))]


def _start(shape, dtype, opts, device, shapes=None, **flat_kw):
    """An optimizer at step 6 with a positive random state, and its gradient."""
    zero = shape == "zero"
    shape = (20, 25) if zero else shape
    # the vector: a chunk plus a scalar tail beside (33, 260), shape[0] elements otherwise
    shapes = shapes or [shape, (8193,) if shape == (33, 260) else (shape[0],)]
    flat = make_flat(shapes=shapes, seed=3, device=device, **flat_kw)
    grad = make_grad(flat, 0, dtype)
    if zero:
        grad[:shape[0] * shape[1]] = 0
    opt = FlatAdafactor(flat, **KW, **dict(opts))
    gen = torch.Generator().manual_seed(11)
    for s in (opt.row, opt.col, opt.v, opt.m):
        if s is not None:
            s.copy_(torch.rand(s.shape, generator=gen) * 0.1 + 1e-3)
    opt.steps = 6
    if opt.step_t is not None:
        opt.step_t.fill_(6)
    return flat, grad, opt


def _state(flat, opt):
    return [flat.data.cpu().clone()] + [s.cpu().clone() for s in (opt.row, opt.col, opt.v)]


@functools.lru_cache(maxsize=None)
def _cpu(shape, dtype, opts):
    """(start, the fp32 oracle's, float64's) lists [p, row, col, v] and the tensors' rows."""
    flat, grad, opt = _start(shape, dtype, opts, "cpu")
    start = _state(flat, opt)
    s64 = [x.double() for x in start]
    m64 = opt.m.double() if opt.m is not None else None
    oracle.adafactor_apply(s64[0], s64[1], s64[2], s64[3], m64, grad.double() * 0.5,
                           opt._tensors(0, flat.numel), step=7, **KW, **dict(opts))
    opt.step(grad=grad, grad_scale=0.5)
    return start, _state(flat, opt), s64, opt._tensors(0, flat.numel)


def _hip(shape, dtype, opts):
    ops.require()
    flat, grad, opt = _start(shape, dtype, opts, "cuda")
    opt.step_range(0, flat.numel, grad, 0.5)
    torch.cuda.synchronize()
    return _state(flat, opt)


@pytest.mark.parametrize("shape,dtype,opts", CASES, ids=str)
def test_one_step_against_float64(shape, dtype, opts):
    start, s32, s64, tensors = _cpu(shape, dtype, opts)
    got = _hip(shape, dtype, opts)
    assert all(bool(torch.isfinite(x).all()) for x in got)
    for off, numel, n, s0, s1 in tensors:
        sl = slice(off, off + numel)
        d64 = s64[0][sl] - start[0][sl].double()
        err = float((got[0][sl].double() - start[0][sl].double() - d64).norm())
        ref = float((s32[0][sl].double() - start[0][sl].double() - d64).norm())
        bound = 3 * ref if ref > 0 else 2.0 ** -23 * float(d64.norm())
        print(f"adafactor {shape} {dtype} {opts} rows={n}: hip {err:.3e} oracle {ref:.3e} "
              f"ratio {err / ref if ref > 0 else float('nan'):.3f}")
        assert err <= bound
        if not n:
            vs = slice(s0, s0 + numel)
            assert torch.equal(got[3][vs].view(torch.int32), s32[3][vs].view(torch.int32)), "v"
            continue
        if shape == "zero":  # u is exactly 0: the parameter only decays
            assert torch.equal(got[0][sl], s32[0][sl])
        rel = (ops.ADAFACTOR_SUM_CHAIN + 4) * 2.0 ** -24
        for name, k, s in (("R", 1, slice(s0, s0 + n)), ("C", 2, slice(s1, s1 + numel // n))):
            e = ((got[k][s].double() - s64[k][s]).abs() / s64[k][s]).max()
            print(f"  {name}: max relative error {float(e):.3e} = {float(e) / rel:.3f} of the bound")
            assert float(e) <= rel, name


def _steps(graph):
    """Two steps of (500, 800), eager or as two replays of one captured step."""
    flat, grad, opt = _start((500, 800), F32, (), "cuda")

    def one():
        opt.step_range(0, flat.numel, grad, 0.5)
        opt.end_step()

    if graph:
        keep = _state(flat, opt)
        one()  # warm up, then back to the start
        for dst, src in zip((flat.data, opt.row, opt.col, opt.v), keep):
            dst.copy_(src)
        opt.step_t.fill_(6)
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, capture_error_mode="thread_local"):
            one()
        g.replay()
        g.replay()
    else:
        one()
        one()
    torch.cuda.synchronize()
    return _state(flat, opt)


def test_two_captured_replays_equal_two_eager_steps():
    """The step counter advances between the replays: beta2_t is read on the device."""
    for a, b in zip(_steps(False), _steps(True)):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32))


def test_bucket_by_bucket_equals_the_whole_model():
    shapes = [(33, 260), (33,), (20, 25), (8193,)]
    out = []
    for whole in (True, False):
        flat, grad, opt = _start(None, F32, (), "cuda", shapes=shapes,
                                 bucket_bytes=4 * 33 * 260)
        assert len(flat.buckets) == 2
        for start, length in [(0, flat.numel)] if whole else [(b.start, b.length)
                                                              for b in flat.buckets]:
            opt.step_range(start, length, grad[start:start + length], 0.5)
        torch.cuda.synchronize()
        out.append(_state(flat, opt))
    for a, b in zip(*out):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32))
