"""``k_outer_apply`` (``ops/csrc/outer.hip``) on one MI355X: bitwise ``oracle.outer_apply`` run on
the CPU for the anchor, the weights, the momentum and the bf16 shadow, and its per-row sums of
squares against float64.

Sizes: 4 (a tail and nothing else), 8188 / 8192 / 8196 (either side of a row boundary) and
3 * 8192 + 20 (several rows and a tail).  The inputs hold +0, -0, a denormal and, in the delta,
one inf; the kernel has no special cases, so the oracle's result is the expectation.  Every
buffer is a view into a larger one whose remainder holds a sentinel: nothing past ``n`` may change.

Bound of the sums.  As for ``k_clip_norm``'s partials (tests/kernels/test_clip_hip.py): a row's
sum is a sum of non-negative squares, each rounded once, through a chain of at most L =
``ops.CLIP_SUM_CHAIN`` fp32 additions, so it is within (L + 1) 2^-24 relative of the float64 sum
of the squares of the same fp32 values.
"""
import pytest
import torch

from ewdml import ops
from ewdml.compress import oracle

pytestmark = pytest.mark.gpu

DEV = "cuda"
SIZES = [4, 8188, 8192, 8196, 3 * 8192 + 20]
SETTINGS = [(1.0, 0.0), (0.7, 0.9), (1.0, 0.9), (0.7, 0.0)]  # (lr, mu)
GUARD = 64
SENTINEL = -1536.0  # exact in bf16 too
U = 2.0 ** -24


def _inputs(n, inf=True):
    g = torch.Generator().manual_seed(n)
    d = torch.randn(n, generator=g) * 0.1
    m = torch.randn(n, generator=g)
    a = torch.randn(n, generator=g)
    for t, k in ((d, 0), (m, 1), (a, 2)):
        t[k % n] = 0.0
        t[(k + 1) % n] = -0.0
        t[(k + 2) % n] = 1e-41  # a denormal
    if inf:
        d[n - 1] = float("inf")
    return a, m, d


def _guarded(t, dtype=None):
    buf = torch.full((t.numel() + GUARD,), SENTINEL, dtype=dtype or t.dtype, device=DEV)
    buf[:t.numel()] = t.to(DEV)
    return buf, buf[:t.numel()]


def _bits(t):
    return t.contiguous().view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32)


@pytest.mark.parametrize("kind", ["sgd", "nesterov"])
@pytest.mark.parametrize("n", SIZES)
def test_kernel_is_bitwise_the_oracle(n, kind):
    ops.require()
    nest = kind == "nesterov"
    rows = ops.outer_rows(n)
    for lr, mu in SETTINGS:
        for with_shadow in (False, True):
            a, m, d = _inputs(n)
            ra, rm, rp = a.clone(), m.clone(), torch.zeros(n)
            rs = torch.zeros(n, dtype=torch.bfloat16) if with_shadow else None
            oracle.outer_apply(ra, rp, rm, d, lr, mu, nest, shadow=rs)
            (ab, av), (mb, mv), (db, dv) = _guarded(a), _guarded(m), _guarded(d)
            pb, pv = _guarded(torch.zeros(n))
            sb, sv = _guarded(torch.zeros(n), torch.bfloat16) if with_shadow else (None, None)
            stats = torch.full((rows + 1, 2), SENTINEL, device=DEV)
            ops.outer_apply(av, pv, mv, dv, lr, mu, nest, shadow=sv, stats=stats[:rows])
            torch.cuda.synchronize()
            tag = f"n={n} {kind} lr={lr} mu={mu} shadow={with_shadow}"
            assert torch.equal(_bits(av.cpu()), _bits(ra)), tag
            assert torch.equal(_bits(pv.cpu()), _bits(ra)), tag
            assert torch.equal(_bits(mv.cpu()), _bits(rm)), tag
            assert torch.equal(_bits(dv.cpu()), _bits(d)), tag  # the delta is only read
            if with_shadow:
                # nesterov with mu = 0 turns the inf into inf + inf * 0 = NaN.  fp32 NaNs are
                # compared by their bits above; a bf16 NaN is only required to be one, since the
                # kernels' conversion (ew_f2bf: the top 16 bits, quieted) and torch's CPU cast
                # keep different payloads
                got, nan = sv.cpu(), rs.isnan()
                assert torch.equal(got.isnan(), nan), tag
                assert torch.equal(_bits(got)[~nan], _bits(rs)[~nan]), tag
                assert bool((sb[n:].float() == SENTINEL).all()), tag
            for buf in (ab, mb, db, pb):
                assert bool((buf[n:] == SENTINEL).all()), tag
            assert bool((stats[rows:] == SENTINEL).all()), tag
            # the sums: the delta's, and the new momentum's as the kernel stored it
            bound = (ops.CLIP_SUM_CHAIN + 1) * U
            got = stats[:rows].cpu().double()
            for k, v in enumerate((d, rm)):
                for r in range(rows):
                    want = float((v[r * 8192:(r + 1) * 8192].double() ** 2).sum())
                    if want == float("inf"):
                        assert float(got[r, k]) == want, tag
                    else:
                        assert abs(float(got[r, k]) - want) <= bound * want, (tag, r, k)


def test_sums_are_within_the_clip_tree_bound_on_finite_inputs():
    """No inf anywhere, so every row's figure is a number: the worst relative error is printed
    and the norms the exchange reports follow from the rows in float64."""
    ops.require()
    n = SIZES[-1]
    a, m, d = _inputs(n, inf=False)
    rm, ra = m.clone(), a.clone()
    oracle.outer_apply(ra, torch.zeros(n), rm, d, 0.7, 0.9, True)
    rows = ops.outer_rows(n)
    stats = torch.zeros((rows, 2), device=DEV)
    ops.outer_apply(a.to(DEV), torch.zeros(n, device=DEV), m.to(DEV), d.to(DEV), 0.7, 0.9, True,
                    stats=stats)
    got = stats.cpu().double()
    worst = 0.0
    for k, v in enumerate((d, rm)):
        for r in range(rows):
            want = float((v[r * 8192:(r + 1) * 8192].double() ** 2).sum())
            worst = max(worst, abs(float(got[r, k]) - want) / want)
        norm = float(torch.sqrt(got[:, k].sum()))
        ref = float(v.double().norm())
        assert abs(norm - ref) <= (ops.CLIP_SUM_CHAIN + 1) * U * ref
    bound = (ops.CLIP_SUM_CHAIN + 1) * U
    print(f"worst relative error of a row's sum {worst:.3e} (bound {bound:.3e})")
    assert ops.CLIP_SUM_CHAIN == 41 and worst <= bound


def test_two_captured_launches_replayed_twice_equal_four_eager_ones():
    ops.require()
    n = SIZES[-1]
    a, m, d = _inputs(n)
    rows = ops.outer_rows(n)

    def state():
        return dict(a=a.to(DEV), m=m.to(DEV), d=d.to(DEV), p=torch.zeros(n, device=DEV),
                    s=torch.zeros(n, dtype=torch.bfloat16, device=DEV),
                    st=torch.zeros((rows, 2), device=DEV))

    def launch(s):
        ops.outer_apply(s["a"], s["p"], s["m"], s["d"], 0.7, 0.9, True, shadow=s["s"],
                        stats=s["st"])

    eager, graphed = state(), state()
    for _ in range(4):
        launch(eager)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        launch(graphed)
        launch(graphed)
    g.replay()
    g.replay()
    torch.cuda.synchronize()
    for k in ("a", "m", "p", "s", "st"):
        assert torch.equal(_bits(graphed[k]), _bits(eager[k])), k
    assert not torch.equal(graphed["a"].cpu()[:n - 1], a[:n - 1])


def test_argument_checks():
    ops.require()
    n = 8192
    t = [torch.zeros(n, device=DEV) for _ in range(4)]
    with pytest.raises(ValueError):
        ops.outer_apply(t[0], t[1], t[2], t[3][:n - 4], 1.0, 0.0, False)
    with pytest.raises(ValueError):
        ops.outer_apply(t[0], t[0], t[2], t[3], 1.0, 0.0, False)
    with pytest.raises(ValueError):
        ops.outer_apply(t[0], t[1], t[2], t[3][1:], 1.0, 0.0, False)  # not 16-byte aligned
    with pytest.raises(TypeError):
        ops.outer_apply(t[0], t[1], t[2].double(), t[3], 1.0, 0.0, False)
    with pytest.raises(ValueError):
        ops.outer_apply(t[0], t[1], t[2], t[3], 1.0, 0.0, False,
                        stats=torch.zeros((2, 2), device=DEV))
    with pytest.raises(ValueError):
        ops.outer_apply(t[0], t[1], t[2], t[3], 0.0, 0.0, False)
    with pytest.raises(ValueError):
        ops.outer_apply(t[0], t[1], t[2], t[3], 1.0, 1.0, False)
    with pytest.raises(ValueError):
        ops.outer_apply(t[0].cpu(), t[1], t[2], t[3], 1.0, 0.0, False)
