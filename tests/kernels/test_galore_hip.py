"""GaLore's kernels (ops/csrc/galore.hip) through ``FlatGalore.step_range`` on the GPU, against
``compress/oracle.py galore_apply`` in float64.  One step (the 7th) from a preloaded positive
state over a flat buffer of one matrix and one vector, ``grad_scale = 0.5``.

Step: with D = new - old of p, M and V per tensor, ``|D_hip - D_64| <= 3 |D_oracle32 - D_64|`` in
norm, the oracle's own fp32 error being the yardstick (floor ``2^-23 |D_64|``); a dense tensor is
element-wise and bitwise the fp32 oracle's.

Refresh (step ``T + 1``, T = 6): the projector's ``|P P^T - P_64 P_64^T|_F`` and ``max |P^T P -
I|`` are each at most 3 times the fp32 oracle's own.  The gradient has ``rank`` singular values in
[1, 2] and the rest at most 1/4, or exact rank ``rank / 2`` (seed 21: every kept column's norm
ratio is above 0.02 and every dropped one's below 1e-13 in float64, the threshold being 2^-12; the
test asserts the factor 16 on both sides).  The ratios are printed."""
import functools

import pytest
import torch

from ewdml import ops
from ewdml.compress import oracle
from ewdml.optim import FlatGalore
from tests.layerwise_ref import make_flat, make_grad

pytestmark = pytest.mark.gpu

KW = dict(lr=1e-2, weight_decay=1e-2)
F32, BF16 = torch.float32, torch.bfloat16
# s one past r, ragged strip | the other orientation | s == r: dense | LeNet conv2 | several
# k-steps, both sides ragged | many strips, unaligned rows | tall, many slabs | the largest rank
SHAPES = [((17, 40), 16), ((40, 17), 16), ((16, 40), 16), ((50, 500), 16), ((500, 800), 32),
          ((33, 4609), 32), ((1030, 70), 64), ((200, 260), 128)]
CASES = [(s, r, F32, "") for s, r in SHAPES] + [((50, 500), 16, BF16, ""), (
    (1030, 70), 64, BF16, ""), ((50, 500), 16, F32, "zero")]
REFRESH = [((40, 17), 16), ((500, 800), 32), ((33, 4609), 32)]
NAMES = ("p", "M", "V")


def _spectrum(shape, rank, kind, gen):
    """A float64 gradient with ``rank`` singular values in [1, 2] and the rest <= 1/4 ("gap"), or
    of exact rank ``rank / 2`` ("deficient")."""
    n, m = shape
    if kind == "deficient":
        return (torch.randn(n, rank // 2, generator=gen, dtype=torch.float64)
                @ torch.randn(rank // 2, m, generator=gen, dtype=torch.float64)) / rank
    k = min(n, m)
    U = torch.linalg.qr(torch.randn(n, k, generator=gen, dtype=torch.float64))[0]
    W = torch.linalg.qr(torch.randn(m, k, generator=gen, dtype=torch.float64))[0]
    sv = torch.cat([torch.linspace(2, 1, rank), torch.linspace(0.25, 0.01, k - rank)]).double()
    return (U * sv) @ W.t()


def _start(shape, rank, dtype, kind, device, gap=100, shapes=None, **flat_kw):
    """An optimizer at step 6 with orthonormal projectors and a positive random state, and its
    gradient."""
    flat = make_flat(shapes=shapes or [shape, (shape[0],)], seed=3, device=device, **flat_kw)
    grad = make_grad(flat, 0, dtype)
    gen = torch.Generator().manual_seed(21)
    if kind == "zero":
        grad[:shape[0] * shape[1]] = 0
    elif kind:  # grad_scale halves it again
        grad[:shape[0] * shape[1]] = (2 * _spectrum(shape, rank, kind, gen)).reshape(-1)
    opt = FlatGalore(flat, rank=rank, update_gap=gap, **KW)
    for t, (s, r) in enumerate(zip(opt.rows, opt._whole.projected)):
        if r and not kind:  # the refresh cases start from the Gaussian
            sl = slice(opt._whole.p0[t], opt._whole.p0[t + 1])
            P = opt.proj[sl].cpu().view(-1, rank)
            opt.proj[sl] = oracle.galore_orth(P).reshape(-1).to(device)
    for s in (opt.m_lr, opt.v_lr, opt.m, opt.v):
        s.copy_(torch.rand(s.shape, generator=gen) * 0.1 + 1e-3)
    opt.steps = 6
    if opt.step_t is not None:
        opt.step_t.fill_(6)
    return flat, grad, opt


def _state(flat, opt):
    return [x.cpu().clone() for x in (flat.data, opt.proj, opt.m_lr, opt.v_lr, opt.m, opt.v)]


@functools.lru_cache(maxsize=None)
def _cpu(shape, rank, dtype, kind, gap):
    """(start, the fp32 oracle's, float64's) states, the tensors' rows, float64's norm ratios."""
    flat, grad, opt = _start(shape, rank, dtype, kind, "cpu", gap)
    start = _state(flat, opt)
    s64 = [x.double() for x in start]
    tensors = opt._tensors(0, flat.numel)
    oracle.galore_apply(*s64, grad.double() * 0.5, tensors, step=7, rank=rank, update_gap=gap,
                        **KW)
    ratios = []
    if kind and kind != "zero":
        n, m = shape
        G = (grad[:n * m].double() * 0.5).view(n, m)
        oracle.galore_refresh(G if n <= m else G.t(), start[1].double().view(-1, rank), 2, ratios)
    opt.step(grad=grad, grad_scale=0.5)
    return start, _state(flat, opt), s64, tensors, ratios


def _hip(shape, rank, dtype, kind, gap):
    ops.require()
    flat, grad, opt = _start(shape, rank, dtype, kind, "cuda", gap)
    opt.step_range(0, flat.numel, grad, 0.5)
    torch.cuda.synchronize()
    return _state(flat, opt)


def _check_step(tag, start, s32, s64, got, tensors, rank, factor=3.0):
    """The update bound per tensor on p, M and V; a dense tensor bitwise."""
    for off, numel, n, p0, s0 in tensors:
        low = rank * max(n, numel // n) if n else numel
        where = [(0, slice(off, off + numel))] + [(k + (0 if n else 2), slice(s0, s0 + low))
                                                  for k in (2, 3)]
        for name, (k, sl) in zip(NAMES, where):
            d64 = s64[k][sl] - start[k][sl].double()
            err = float((got[k][sl].double() - start[k][sl].double() - d64).norm())
            ref = float((s32[k][sl].double() - start[k][sl].double() - d64).norm())
            print(f"galore {tag} rows={n} {name}: hip {err:.3e} oracle {ref:.3e} ratio "
                  f"{err / ref if ref > 0 else float('nan'):.3f}")
            assert err <= max(factor * ref, 2.0 ** -23 * float(d64.norm())), name
            if not n:
                bad = int((got[k][sl].view(torch.int32) != s32[k][sl].view(torch.int32)).sum())
                assert bad == 0, f"dense {name}: {bad} of {numel} elements differ"


@pytest.mark.parametrize("shape,rank,dtype,kind", CASES, ids=str)
def test_one_step_against_float64(shape, rank, dtype, kind):
    start, s32, s64, tensors, _ = _cpu(shape, rank, dtype, kind, 100)
    got = _hip(shape, rank, dtype, kind, 100)
    assert all(bool(torch.isfinite(x).all()) for x in got)
    assert torch.equal(got[1], start[1]), "no refresh at this step"
    _check_step(f"{shape} r={rank} {dtype} {kind}", start, s32, s64, got, tensors, rank)


@pytest.mark.parametrize("kind", ["gap", "deficient"])
@pytest.mark.parametrize("shape,rank", REFRESH, ids=str)
def test_refresh_against_float64(shape, rank, kind):
    start, s32, s64, tensors, ratios = _cpu(shape, rank, F32, kind, 6)
    got = _hip(shape, rank, F32, kind, 6)
    P, P32, P64 = (x[1].double().view(-1, rank) for x in (got, s32, s64))
    zero = [bool((x == 0).all(dim=0)[c]) for x in (P, P64) for c in range(rank)]
    assert zero[:rank] == zero[rank:]
    if kind == "deficient":
        assert sum(zero[:rank]) == rank // 2
        assert all(x > 16 * oracle.GALORE_ZERO or x < oracle.GALORE_ZERO / 16 for x in ratios)
    kept = torch.tensor([0.0 if z else 1.0 for z in zero[:rank]], dtype=torch.float64)
    dist = [float((x @ x.t() - P64 @ P64.t()).norm()) for x in (P, P32)]
    defect = [float((x.t() @ x - torch.diag(kept)).abs().max()) for x in (P, P32)]
    print(f"galore refresh {shape} r={rank} {kind}: distance hip {dist[0]:.3e} oracle "
          f"{dist[1]:.3e} ratio {dist[0] / dist[1]:.3f}; defect hip {defect[0]:.3e} oracle "
          f"{defect[1]:.3e} ratio {defect[0] / defect[1]:.3f}")
    assert dist[0] <= 3 * dist[1] and defect[0] <= 3 * defect[1]


def _run(mode):
    """Five steps with a refresh at steps 1 and 4 over two buckets: the whole model eagerly
    ("whole"), bucket by bucket ("buckets"), or one captured step replayed ("graph")."""
    shapes = [(33, 260), (33,), (40, 17), (8193,)]
    flat, _, opt = _start(None, 16, F32, "", "cuda", gap=3, shapes=shapes,
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

    graph = None
    if mode == "graph":
        one()  # warm up, then back to the start
        for dst, src in zip((flat.data, opt.proj, opt.m_lr, opt.v_lr, opt.m, opt.v), keep):
            dst.copy_(src)
        opt.step_t.fill_(0)
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, capture_error_mode="thread_local"):
            one()
        for dst, src in zip((flat.data, opt.proj, opt.m_lr, opt.v_lr, opt.m, opt.v), keep):
            dst.copy_(src)
        opt.step_t.fill_(0)
    for t in range(5):
        gbuf.copy_(make_grad(flat, t))
        graph.replay() if graph else one()
    torch.cuda.synchronize()
    return _state(flat, opt)


def test_buckets_graph_and_reruns_are_bitwise_the_eager_whole_model():
    want = _run("whole")
    for mode in ("whole", "buckets", "graph"):
        for name, a, b in zip(("p", "proj", "m_lr", "v_lr", "m", "v"), want, _run(mode)):
            assert torch.equal(a.view(torch.int32), b.view(torch.int32)), (mode, name)
