"""APOLLO's kernels (ops/csrc/apollo.hip) through ``FlatApollo.step_range`` on the GPU, against
``compress/oracle.py apollo_apply`` in float64.  One step (the 7th) from a preloaded positive
state and a preloaded previous norm over a flat buffer of one matrix and one vector, ``grad_scale
= 0.5``.

With D = new - old of p, M and V per tensor, ``|D_hip - D_64| <= 3 |D_oracle32 - D_64|`` in norm,
the oracle's own fp32 error being the yardstick (floor ``2^-23 |D_64|``); a dense tensor is
element-wise and bitwise the fp32 oracle's.  The projection's signs are exact in both precisions,
so a kernel whose bits differ from the oracle's misses the bound on M by orders of magnitude.

The previous norm is ``prev`` times float64's own update norm u (1 where u is 0), so the limiter
is ``max(1 / prev, 1.01) / 1.01``: on at 1/2 and 1/4, off at 4, never near its kink.  The stored
norm is a single fp32 number, a root of a sum of at most 4609 fp32 terms: it is held to 1e-4 of
float64's, where the wrong parity slot, a wrong limiter or one strip left out of 73 are off by
1e-2 or more.  The ratios are printed."""
import functools

import pytest
import torch

from ewdml import ops
from ewdml.compress import oracle
from ewdml.optim import FlatApollo
from tests.layerwise_ref import make_flat, make_grad

pytestmark = pytest.mark.gpu

KW = dict(lr=1e-2, weight_decay=1e-2, seed=5)
F32, BF16 = torch.float32, torch.bfloat16
# (shape, rank, scale type, gradient dtype, kind, previous norm over u)
CASES = [
    ((17, 40), 16, "channel", F32, "", 0.5),      # s one past r, ragged strip
    ((40, 17), 16, "channel", F32, "", 0.5),      # the tall orientation
    ((16, 40), 16, "channel", F32, "", 0.5),      # s == r: dense, bitwise
    ((50, 500), 16, "channel", F32, "", 0.5),     # LeNet conv2
    ((500, 800), 32, "channel", F32, "", 0.5),    # many panels, both sides ragged
    ((33, 4609), 32, "channel", F32, "", 0.5),    # 73 strip partials, unaligned rows
    ((200, 260), 128, "channel", F32, "", 0.5),   # the largest rank
    ((20, 70), 1, "tensor", F32, "", 0.5),        # rank 1, masked rows
    ((50, 500), 16, "tensor", F32, "", 0.5),      # tensor scale
    ((50, 500), 16, "channel", BF16, "", 0.5),    # bf16 loads
    ((50, 500), 16, "channel", F32, "zero", 0.5), # p only decays, the stored norm becomes 0
    ((50, 500), 16, "channel", F32, "", 0.25),    # limiter on: lim = 4 / 1.01
    ((50, 500), 16, "channel", F32, "", 4.0),     # limiter off: lim = 1
]
NAMES = ("p", "M", "V")
STATE = ("m_lr", "v_lr", "m", "v", "norms")


def _start(shape, rank, stype, dtype, kind, device, gap=100, shapes=None, **flat_kw):
    """An optimizer at step 6 with a positive random state, and its gradient."""
    flat = make_flat(shapes=shapes or [shape, (shape[0],)], seed=3, device=device, **flat_kw)
    grad = make_grad(flat, 0, dtype)
    if kind == "zero":
        grad[:shape[0] * shape[1]] = 0
    opt = FlatApollo(flat, rank=rank, update_gap=gap, scale_type=stype, **KW)
    gen = torch.Generator().manual_seed(21)
    for s in (opt.m_lr, opt.v_lr, opt.m, opt.v):
        s.copy_(torch.rand(s.shape, generator=gen) * 0.1 + 1e-3)
    opt.steps = 6
    if opt.step_t is not None:
        opt.step_t.fill_(6)
    return flat, grad, opt


def _state(flat, opt):
    return [x.cpu().clone() for x in (flat.data, *(getattr(opt, k) for k in STATE))]


@functools.lru_cache(maxsize=None)
def _cpu(shape, rank, stype, dtype, kind, prev):
    """(start, the fp32 oracle's, float64's) states, the tensors' rows and float64's limiter."""
    flat, grad, opt = _start(shape, rank, stype, dtype, kind, "cpu")
    tensors = opt._tensors(0, flat.numel)
    hp = dict(step=7, rank=rank, update_gap=100, scale_type=stype, **KW)
    if opt.norms.numel():
        # float64's u: the norm stored by a step that has no previous one
        probe = [x.double() for x in _state(flat, opt)]
        oracle.apollo_apply(*probe, grad.double() * 0.5, tensors, **hp)
        u = float(probe[5][1])
        opt.norms[0] = prev * u if u > 0 else 1.0  # step 7 reads slot 0 and writes slot 1
    start = _state(flat, opt)
    s64 = [x.double() for x in start]
    oracle.apollo_apply(*s64, grad.double() * 0.5, tensors, **hp)
    opt.step(grad=grad, grad_scale=0.5)
    lim = u / float(s64[5][1]) if opt.norms.numel() and u > 0 else None  # it stored u / lim
    return start, _state(flat, opt), s64, tensors, lim


def _hip(shape, rank, stype, dtype, kind, norms):
    ops.require()
    flat, grad, opt = _start(shape, rank, stype, dtype, kind, "cuda")
    opt.norms.copy_(norms)
    opt.step_range(0, flat.numel, grad, 0.5)
    torch.cuda.synchronize()
    return _state(flat, opt)


@pytest.mark.parametrize("shape,rank,stype,dtype,kind,prev", CASES, ids=str)
def test_one_step_against_float64(shape, rank, stype, dtype, kind, prev):
    start, s32, s64, tensors, lim = _cpu(shape, rank, stype, dtype, kind, prev)
    got = _hip(shape, rank, stype, dtype, kind, start[5])
    tag = f"apollo {shape} r={rank} {stype} {dtype} {kind} prev={prev}"
    assert all(bool(torch.isfinite(x).all()) for x in got)
    for off, numel, n, gidx, s0, k in tensors:
        low = rank * max(n, numel // n) if n else numel
        where = [(0, slice(off, off + numel))] + [(i + (0 if n else 2), slice(s0, s0 + low))
                                                  for i in (1, 2)]
        for name, (i, sl) in zip(NAMES, where):
            d64 = s64[i][sl] - start[i][sl].double()
            err = float((got[i][sl].double() - start[i][sl].double() - d64).norm())
            ref = float((s32[i][sl].double() - start[i][sl].double() - d64).norm())
            print(f"{tag} rows={n} {name}: hip {err:.3e} oracle {ref:.3e} ratio "
                  f"{err / ref if ref > 0 else float('nan'):.3f}")
            assert err <= max(3.0 * ref, 2.0 ** -23 * float(d64.norm())), name
            if not n:
                bad = int((got[i][sl].view(torch.int32) != s32[i][sl].view(torch.int32)).sum())
                assert bad == 0, f"dense {name}: {bad} of {numel} elements differ"
        if n:
            want = float(s64[5][2 * k + 1])
            print(f"{tag} norm: hip {float(got[5][2 * k + 1]):.7e} float64 {want:.7e} lim {lim}")
            assert got[5][2 * k] == start[5][2 * k], "the slot that was read stays"
            assert abs(float(got[5][2 * k + 1]) - want) <= 1e-4 * want
            if kind == "zero":
                assert want == 0 and lim is None
            else:  # the limiter float64 took is the one the case is about (prev u is an fp32)
                assert abs(lim - max(1 / prev, 1.01) / 1.01) <= 1e-6 * lim


def _run(mode):
    """Five steps over two buckets with the signs redrawn at step 4 from the device counter: the
    whole model eagerly ("whole"), bucket by bucket ("buckets"), or one captured step replayed
    ("graph")."""
    shapes = [(33, 260), (33,), (40, 17), (8193,)]
    flat, _, opt = _start(None, 16, "channel", F32, "", "cuda", gap=3, shapes=shapes,
                          bucket_bytes=4 * 33 * 260)
    assert len(flat.buckets) == 2
    opt.steps = 0
    opt.step_t.fill_(0)
    keep = _state(flat, opt)
    gbuf = make_grad(flat, 0)
    ranges = ([(b.start, b.length) for b in flat.buckets] if mode == "buckets"
              else [(0, flat.numel)])

    def one():
        for start, length in ranges:
            opt.step_range(start, length, gbuf[start:start + length], 0.5)
        opt.end_step()

    def rewind():
        for dst, src in zip((flat.data, *(getattr(opt, k) for k in STATE)), keep):
            dst.copy_(src)
        opt.step_t.fill_(0)

    graph = None
    if mode == "graph":
        one()  # warm up, then back to the start
        rewind()
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, capture_error_mode="thread_local"):
            one()
        rewind()
    for t in range(5):
        gbuf.copy_(make_grad(flat, t))
        graph.replay() if graph else one()
    torch.cuda.synchronize()
    return _state(flat, opt)


def test_buckets_graph_and_reruns_are_bitwise_the_eager_whole_model():
    want = _run("whole")
    assert bool((want[5] > 0).all()), "both slots of both matrices were written"
    for mode in ("whole", "buckets", "graph"):
        for name, a, b in zip(("p",) + STATE, want, _run(mode)):
            assert torch.equal(a.view(torch.int32), b.view(torch.int32)), (mode, name)
