"""PowerSGD on the CPU: the low-rank plan, the oracle's properties in fp64, error feedback, and the
command line (``--compress powersgd``)."""
import pytest
import torch

import ewdml
from ewdml.compress import make_codec, oracle
from ewdml.compress.plan import LowRankPlan
from tests.powersgd_sim import make_plan, numel, rel, same_bits

LENET = [(20, 1, 5, 5), (20,), (50, 20, 5, 5), (50,), (500, 800), (500,), (10, 500), (10,)]
PLAN_SHAPES = [(20, 1, 5, 5), (50, 20, 5, 5), (500, 800), (10, 500), (64, 3, 3, 3),
               (20,), (50,), (500,), (10,)]


def _nm(s):
    return s[0], numel(s) // s[0]


@pytest.mark.parametrize("r", [1, 2, 4, 8])
def test_plan_compresses_by_the_rule_and_packs_the_factors(r):
    lrp, length = make_plan(PLAN_SHAPES, r, bucket_offset=128)
    want = [t for t, s in enumerate(PLAN_SHAPES)
            if len(s) >= 2 and numel(s) >= 2 * r * sum(_nm(s))]
    assert lrp.compressed == want
    if r == 8:  # [20, 25] (500 < 720) and [10, 500] (5000 < 8160) are too small for rank 8;
        assert want == [1, 2, 4]  # [64, 27] still passes: 1728 >= 16 * 91 = 1456
    else:
        assert want == [0, 1, 2, 3, 4]
    p = q = 0
    for (off, n, m, po, qo, t), per in zip(lrp.mats, lrp.split):
        assert (n, m) == _nm(PLAN_SHAPES[t]) and off == lrp.plan.offsets[t]
        assert (po, qo) == (p, q) and min(n, m) > 2 * r
        p, q = p + n * r, q + m * r
    assert lrp.p_factor_floats == p and lrp.q_floats == q
    dense = [t for t in range(len(PLAN_SHAPES)) if t not in want]
    assert [t for *_, t in lrp.dense] == dense
    for off, n_el, tail, t in lrp.dense:
        assert off == lrp.plan.offsets[t] and n_el == numel(PLAN_SHAPES[t]) and tail == p
        p += n_el
    assert lrp.p_floats == p
    # every element of every matrix is in exactly one project item and one tile item per split
    rows = sum(b for k, _, _, b in lrp.row_items if k == 0)
    assert rows == sum(n for _, n, *_ in lrp.mats)
    assert sum(b for k, _, _, b in lrp.row_items if k == 1) == sum(n for _, n, _, _ in lrp.dense)
    assert lrp.mat_table("cpu").shape[1] == 12 and lrp.row_table("cpu").shape[1] == 4


def test_plan_totals_of_lenet_and_refusals():
    for r, total in ((4, 10200), (1, 2985)):
        lrp, _ = make_plan(LENET, r)
        assert lrp.p_floats + lrp.q_floats == total
    with pytest.raises(ValueError, match="rank"):
        make_plan(LENET, 3)
    lrp, _ = make_plan(LENET, 4)
    with pytest.raises(ValueError, match="128"):
        from ewdml.compress.plan import BucketPlan

        LowRankPlan(BucketPlan([1] * 129, [64 * i for i in range(129)]), [(1,)] * 129, 4)


def _factors(shapes, r, seed=0):
    lrp, length = make_plan(shapes, r)
    gen = torch.Generator().manual_seed(seed)
    return lrp, length, gen


def test_orthogonalize_gives_orthonormal_columns_fp64():
    lrp, length, gen = _factors([(60, 40), (9,), (33, 70)], 4)
    p = torch.randn(lrp.p_floats, generator=gen, dtype=torch.float64)
    tail = p[lrp.p_factor_floats:].clone()
    oracle.powersgd_orthogonalize(p, lrp, 1.0 / 3, torch.float64)
    for _, n, _, po, _, _ in lrp.mats:
        P = p[po:po + n * 4].view(n, 4)
        assert float((P.t() @ P - torch.eye(4, dtype=torch.float64)).abs().max()) < 1e-7
    assert torch.equal(p[lrp.p_factor_floats:], tail)


def test_exact_low_rank_matrix_is_reconstructed_after_two_steps_fp64():
    r, dt = 4, torch.float64
    lrp, length, gen = _factors([(60, 40), (9,)], r)
    off, n, m = lrp.mats[0][:3]
    g = torch.zeros(length, dtype=dt)
    # rank exactly r: a rank-deficient P leaves Gram-Schmidt a column of rounding noise, which
    # the non-zero epsilon (torch's rule) does not normalise to a unit vector
    low = torch.randn(n, r, generator=gen, dtype=dt) @ torch.randn(r, m, generator=gen, dtype=dt)
    # col /= (|col| + 1e-8) leaves a column 1e-8 / |col| short of unit length, and g^ = P P^T M
    # inherits that relative error: a gradient of norm ~1e5 puts it at ~1e-12, below the bound
    low *= 1e3
    g[off:off + n * m] = low.reshape(-1)
    g[lrp.dense[0][0]:lrp.dense[0][0] + 9] = torch.arange(9, dtype=dt)
    resid = torch.zeros(length, dtype=dt)
    q = oracle.powersgd_init_q(lrp, 0, 0, dt)
    for _ in range(2):
        ghat = torch.zeros(length, dtype=dt)
        p = oracle.powersgd_project(g, resid, q, lrp, dt)
        oracle.powersgd_orthogonalize(p, lrp, 1.0, dt)
        q = oracle.powersgd_backproject(resid, p, lrp, dt)
        q = oracle.powersgd_reconstruct_apply(resid, p, q, lrp, 1.0, grad_out=ghat, dtype=dt)
    assert rel(ghat[off:off + n * m], low.reshape(-1)) < 1e-10
    assert float(resid.abs().max()) < 1e-10 * float(low.abs().max())
    assert torch.equal(ghat[lrp.dense[0][0]:lrp.dense[0][0] + 9], torch.arange(9, dtype=dt))


def test_residual_plus_ghat_is_m_exactly_and_zero_gradient_stays_zero():
    lrp, length, gen = _factors([(60, 40), (9,), (33, 70)], 2)
    g = torch.randn(length, generator=gen)
    resid = torch.randn(length, generator=gen)
    q = oracle.powersgd_init_q(lrp, 0, 0)
    want_m = g + resid
    before = resid.clone()
    p = oracle.powersgd_project(g, resid, q, lrp)
    M = resid.clone()
    keep = torch.ones(length, dtype=torch.bool)
    for off, n, m, *_ in lrp.mats:  # resid holds M = g + residual on the compressed tensors
        assert torch.equal(M[off:off + n * m], want_m[off:off + n * m])
        keep[off:off + n * m] = False
    assert torch.equal(M[keep], before[keep])  # dense tensors and padding keep no residual
    oracle.powersgd_orthogonalize(p, lrp, 1.0)
    q2 = oracle.powersgd_backproject(resid, p, lrp)
    ghat = torch.zeros(length)
    oracle.powersgd_reconstruct_apply(resid, p, q2, lrp, 1.0, grad_out=ghat)
    for off, n, m, *_ in lrp.mats:
        sl = slice(off, off + n * m)
        # the residual is fl(M - g^), one rounding and nothing else ...
        assert torch.equal(resid[sl], M[sl] - ghat[sl])
        # ... so residual + g^ == M exactly wherever that subtraction is exact (Sterbenz: g^ / 2
        # <= M <= 2 g^), and to half an ulp of the larger operand everywhere else (an element
        # with |M| far below |g^| cannot come back out of fl(M - g^) in any arithmetic)
        a, b = M[sl], ghat[sl]
        exact = (a * b > 0) & (a.abs() <= 2 * b.abs()) & (b.abs() <= 2 * a.abs())
        assert int(exact.sum()) > 0
        assert torch.equal((resid[sl] + b)[exact], a[exact])
        ulp = torch.maximum(a.abs(), b.abs()) * 2.0 ** -23
        assert bool(((resid[sl] + b - a).abs() <= ulp).all())
    # an all-zero gradient: finite, zero P, Q and g^
    z = torch.zeros(length)
    rz = torch.zeros(length)
    p = oracle.powersgd_project(z, rz, q, lrp)
    oracle.powersgd_orthogonalize(p, lrp, 0.5)
    q3 = oracle.powersgd_backproject(rz, p, lrp)
    gz = torch.ones(length)
    qa = oracle.powersgd_reconstruct_apply(rz, p, q3, lrp, 0.5, grad_out=gz)
    for t in (p, q3, qa, rz):
        assert bool(torch.isfinite(t).all()) and float(t.abs().max()) == 0.0
    for off, n, m, *_ in lrp.mats:
        assert float(gz[off:off + n * m].abs().max()) == 0.0


def _ef_errors(dtype, steps=30):
    """Relative error of the running mean of g^ against a constant gradient, per step."""
    lrp, length, gen = _factors([(48, 64), (11,), (40, 3, 3, 3)], 2, seed=5)
    g = torch.randn(length, generator=gen).to(dtype)
    mask = torch.zeros(length, dtype=torch.bool)
    for off, n, m, *_ in lrp.mats:
        mask[off:off + n * m] = True
    resid = torch.zeros(length, dtype=dtype)
    q = oracle.powersgd_init_q(lrp, 1, 0, dtype)
    total = torch.zeros(length, dtype=dtype)
    errs = []
    for s in range(steps):
        ghat = torch.zeros(length, dtype=dtype)
        p = oracle.powersgd_project(g, resid, q, lrp, dtype)
        oracle.powersgd_orthogonalize(p, lrp, 1.0, dtype)
        qs = oracle.powersgd_backproject(resid, p, lrp, dtype)
        q = oracle.powersgd_reconstruct_apply(resid, p, qs, lrp, 1.0, grad_out=ghat, dtype=dtype)
        total += ghat
        errs.append(rel((total / (s + 1))[mask], g.double()[mask]))
    return errs


def test_error_feedback_makes_the_mean_of_ghat_converge():
    e64, e32 = _ef_errors(torch.float64), _ef_errors(torch.float32)
    factor = e64[0] / e64[-1]
    print(f"fp64: error {e64[0]:.4f} at step 1, {e64[-1]:.4f} at step 30 (x{factor:.1f}); "
          f"fp32 {e32[-1]:.4f}")
    assert factor > 1  # mean(g^) = g - residual / steps: the error falls while the residual is bounded
    assert e32[-1] <= 3 * e64[-1] + 1e-5
    assert e32[-1] <= 3 * e32[0] / factor + 1e-5


# ---- command line ------------------------------------------------------------------------------
def test_flags_parse_and_auto_graph_mode():
    c = ewdml.parse_args(["--compress", "powersgd"])
    assert c.compress == "powersgd" and c.powersgd_rank == 4 and c.error_feedback is True
    c = ewdml.parse_args(["--compress", "powersgd", "--powersgd-rank", "8", "--hip-graph", "split"])
    assert c.powersgd_rank == 8
    from ewdml.parallel.engine import plan_graph_mode

    assert plan_graph_mode(1, "local", "powersgd", 431080)["mode"] == "split"
    assert plan_graph_mode(8, "rccl-stream", "powersgd", 431080)["mode"] == "split"


@pytest.mark.parametrize("flags,why", [
    (["--topology", "ps"], "topology ps"),
    (["--topology", "sharded"], "topology sharded"),
    (["--topology", "twostage"], "twostage"),
    (["--sync-every", "4"], "sync-every"),
    (["--select-best"], "select-best"),
    (["--no-error-feedback"], "no-error-feedback"),
    (["--predivide", "2"], "predivide"),
    (["--hip-graph", "full"], "hip-graph full"),
    (["--hip-graph", "segmented"], "hip-graph segmented"),
    (["--optimizer", "onebit_adam", "--onebit-warmup-steps", "3"], "onebit_adam"),
    (["--powersgd-rank", "3"], "powersgd-rank 3"),
])
def test_unsupported_combinations_are_refused_with_a_reason(flags, why):
    with pytest.raises(ValueError, match=why):
        ewdml.parse_args(["--compress", "powersgd"] + flags)


def test_rank_flag_needs_the_codec_and_the_codec_describes_itself():
    with pytest.raises(ValueError, match="powersgd-rank belongs"):
        ewdml.parse_args(["--compress", "sign", "--powersgd-rank", "2"])
    assert make_codec("powersgd").describe() == "powersgd-r4"
    assert make_codec("powersgd", rank=1).describe() == "powersgd-r1"
    with pytest.raises(ValueError, match="rank"):
        make_codec("powersgd", rank=3)


def test_horovod_compression_returns_the_codec_and_the_optimizer_refuses_it():
    import ewdml.parallel.horovod as hvd

    codec = hvd.Compression.powersgd(rank=2)
    assert codec.kind == "powersgd" and codec.rank == 2
    assert hvd.Compression.powersgd().rank == 4
    model = torch.nn.Linear(8, 4)
    with pytest.raises(ValueError, match="--compress powersgd"):
        hvd.DistributedOptimizer(torch.optim.SGD(model.parameters(), lr=0.1),
                                 compression=codec)


def test_one_rank_exchange_on_the_cpu_follows_the_oracle_simulation():
    from tests.powersgd_sim import run_rank, simulate

    out, sim = run_rank(0, 1, 3), simulate(1, 3)
    assert out["buckets"] == 2
    for name in ("params", "mom"):
        assert same_bits(out[name], sim[name]), name
    assert same_bits(out["resid"], sim["resid"][0])
    assert float(out["resid"].abs().max()) > 0
