"""The count-sketch codec on the CPU: the oracle (``compress/oracle.py sketch_*``, also the CPU
execution path) against the independent numpy simulation of ``tests/sketch_sim.py`` bit for bit,
the sketch's exact properties, heavy-hitter recovery, and the configuration."""
import numpy as np
import pytest
import torch

import ewdml
from ewdml.compress import make_codec, oracle
from ewdml.compress.plan import CHUNK, SKETCH_SUM_GROUP, BucketPlan, Layout, SketchPlan

from .. import sketch_sim as S

LR, MOM = 2.0 ** -4, 0.5
HP = dict(lr=LR, momentum=MOM, dampening=0.0, weight_decay=0.0, nesterov=False)


def _grads(n, ranks=2, seed=11):
    gen = torch.Generator().manual_seed(seed)
    out = []
    for _ in range(ranks):
        g = torch.randn(n, generator=gen)
        g[torch.randperm(n, generator=gen)[:n // 50]] *= 30.0  # some heavy coordinates
        out.append(g)
    return out


def _oracle_step(sp, lay, grads, resids, param, mom, first):
    """All ranks through the oracle (sums in rank order), as SimBucket.step."""
    N = len(grads)
    for g, r in zip(grads, resids):
        oracle.sketch_stage(g, r, sp)
    tables = [oracle.sketch_accumulate(r, sp) for r in resids]
    T = tables[0].clone()
    for x in tables[1:]:
        T += x
    est = oracle.sketch_estimate(T, sp)
    pays = []
    for g, r in zip(grads, resids):
        pay = oracle.sketch_select(est, sp, lay)
        oracle.sketch_gather(pay, g, r, sp, lay)
        pays.append(pay)
    vals_r = [oracle._section(p, lay.codes, sp.plan.total_k, torch.float32).clone()
              for p in pays]
    vals = oracle._section(pays[0], lay.codes, sp.plan.total_k, torch.float32)
    for x in vals_r[1:]:
        vals += x
    pos, _ = oracle._decoded_entries(pays[0], sp.plan, lay, 0)
    ghat = oracle.decode_sum(pays[0][None], sp.plan, lay, 0, 1.0 / N)
    for off, n in zip(sp.plan.offsets, sp.plan.numels):
        oracle.sgd_apply(param[off:off + n], mom[off:off + n], ghat[off:off + n], LR, MOM, 0.0,
                         0.0, False, first)
    return {"tables": tables, "table": T, "est": est, "pos": pos, "vals_r": vals_r,
            "vals": vals.clone(), "ghat": ghat}


@pytest.mark.parametrize("width,W", [(1.0, CHUNK), (2.0, 2 * CHUNK)])
@pytest.mark.parametrize("rows", [1, 3, 5])
def test_oracle_equals_the_numpy_simulation_bitwise(rows, width, W):
    sp, lay, sim = S.make_plans(rows, width)
    assert sp.W == sim.W == W
    assert sp.plan.num_chunks > SKETCH_SUM_GROUP  # the group boundary is crossed
    assert sp.dense == [False, False, True, True, False]
    assert sp.shifts == sim.shifts and sp.shifts[0][0] == W - 1 and sp.shifts[0][3] == W - 17
    L = sp.plan.length
    gen = torch.Generator().manual_seed(2)
    p_o, m_o = torch.randn(L, generator=gen), torch.zeros(L)
    p_s, m_s = p_o.numpy().copy(), np.zeros(L, dtype=np.float32)
    r_o = [torch.zeros(L), torch.zeros(L)]
    r_s = [np.zeros(L, dtype=np.float32), np.zeros(L, dtype=np.float32)]
    for step in range(2):  # the second step starts from a non-zero residual and momentum
        grads = _grads(L, seed=11 + step)
        o = _oracle_step(sp, lay, grads, r_o, p_o, m_o, step == 0)
        s = sim.step([g.numpy() for g in grads], r_s, p_s, m_s, LR, MOM, step == 0)
        for r in range(2):
            assert S.same_bits(o["tables"][r], s["tables"][r]), ("table", step, r)
            assert S.same_bits(o["vals_r"][r], s["vals_r"][r]), ("vals", step, r)
            assert S.same_bits(r_o[r], r_s[r]), ("resid", step, r)
        for name in ("table", "est", "vals", "ghat"):
            assert S.same_bits(o[name], s[name]), (name, step)
        assert torch.equal(o["pos"], torch.from_numpy(s["pos"])), step
        assert S.same_bits(p_o, p_s) and S.same_bits(m_o, m_s), step
    assert float(r_o[0].abs().max()) > 0 and not S.same_bits(r_o[0], r_o[1])


def _single(rows, width=2.0):
    sp, lay, _ = S.make_plans(rows, width, edges=False)
    return sp, lay, torch.zeros(sp.plan.length)


@pytest.mark.parametrize("rows", [1, 3, 5])
def test_a_single_nonzero_is_estimated_exactly(rows):
    sp, lay, acc = _single(rows)
    i = 2 * CHUNK + 77
    acc[i] = -3.7
    est = oracle.sketch_estimate(oracle.sketch_accumulate(acc, sp), sp)
    assert S.same_bits(est[i], acc[i])
    if rows == 1:
        # nonzero exactly where a coordinate shares i's column: one per sketched chunk whose image
        # covers it
        col = (i % CHUNK + sp.shifts[0][i // CHUNK]) % sp.W
        share = [start + (col - sp.shifts[0][c]) % sp.W for c, (start, ln) in
                 enumerate(sp.chunk_rows) if (col - sp.shifts[0][c]) % sp.W < ln]
        assert i in share
        assert sorted(share) == est.nonzero().flatten().tolist()


def test_resid_plus_scattered_values_is_acc_and_dense_never_touches_the_table():
    sp, lay, _ = S.make_plans(3, 2.0)
    L = sp.plan.length
    g, resid = _grads(L, 1)[0], _grads(L, 1, seed=5)[0] * 0.1
    for t, d in enumerate(sp.dense):  # dense tensors keep no residual
        if d:
            resid[sp.plan.offsets[t]:sp.plan.offsets[t] + sp.plan.numels[t]] = 0.0
    oracle.sketch_stage(g, resid, sp)
    acc = resid.clone()
    table = oracle.sketch_accumulate(resid, sp)
    # a dense tensor never touches the table: poison its gradient and residual
    poisoned = acc.clone()
    for t, d in enumerate(sp.dense):
        if d:
            poisoned[sp.plan.offsets[t]:sp.plan.offsets[t] + sp.plan.numels[t]] = float("nan")
    assert S.same_bits(table, oracle.sketch_accumulate(poisoned, sp))
    est = oracle.sketch_estimate(table, sp)
    pay = oracle.sketch_select(est, sp, lay)
    oracle.sketch_gather(pay, g, resid, sp, lay)
    pos, vals = oracle._decoded_entries(pay, sp.plan, lay, 0)
    assert [int(((pos >= o) & (pos < o + n)).sum()) for o, n in
            zip(sp.plan.offsets, sp.plan.numels)] == sp.plan.ks
    scat = torch.zeros(L)
    scat[pos] = vals
    want = acc.clone()
    for t, d in enumerate(sp.dense):  # dense tensors: the values are g itself, no residual
        if d:
            sl = slice(sp.plan.offsets[t], sp.plan.offsets[t] + sp.plan.numels[t])
            want[sl] = g[sl]
            assert not resid[sl].any() and not est[sl].any()
    # each side is one value or 0 (x + 0 keeps x's bits unless x is -0.0, which randn never is)
    assert S.same_bits(resid + scat, want)


def test_the_table_is_linear_across_ranks():
    sp, _, _ = S.make_plans(3, 2.0)
    a, b = _grads(sp.plan.length)
    for t, d in enumerate(sp.dense):
        if d:
            sl = slice(sp.plan.offsets[t], sp.plan.offsets[t] + sp.plan.numels[t])
            a[sl] = b[sl] = 0.0
    ta, tb = oracle.sketch_accumulate(a, sp), oracle.sketch_accumulate(b, sp)
    # what the all-reduce gives for two ranks is the elementwise sum of the per-rank tables:
    # every entry is summed per rank first
    world2 = torch.stack([ta, tb]).sum(0)
    assert S.same_bits(ta + tb, world2)
    # and the sketch of the sum, up to fp32 rounding: an entry sums under 128 terms (at most one
    # per chunk and rank), so it is off by less than 128 * 2^-24 of the largest entry's abs-sum,
    # itself under 128 * max|x|
    tsum = oracle.sketch_accumulate(a + b, sp)
    bound = 128 * 2.0 ** -24 * 128 * float(torch.maximum(a.abs(), b.abs()).max())
    err = float((ta + tb - tsum).abs().max())
    print(f"linearity: max error {err:.3e}, bound {bound:.3e}")
    assert err <= bound


RECOVERY_SEED = 5  # chosen on the CPU so that the oracle recovers the spike set exactly


def test_heavy_hitters_are_recovered_exactly():
    n = 4 * CHUNK  # k = 32 spikes, W = 8192
    bp = BucketPlan([n], [0], 0.001, 0, n)
    k = bp.ks[0]
    sp = SketchPlan(bp, 3, 2.0, *oracle.sketch_keys(RECOVERY_SEED, 0))
    lay = Layout.build("topk", bp)
    gen = torch.Generator().manual_seed(RECOVERY_SEED)
    where = torch.randperm(n, generator=gen)[:k]
    acc = torch.zeros(n)
    sign = torch.where(torch.rand(k, generator=gen) < 0.5, -1.0, 1.0)
    acc[where] = sign * (1.0 + torch.arange(k) / k)  # distinct magnitudes in [1, 2)
    est = oracle.sketch_estimate(oracle.sketch_accumulate(acc, sp), sp)
    pos, _ = oracle._decoded_entries(oracle.sketch_select(est, sp, lay), bp, lay, 0)
    assert set(pos.tolist()) == set(where.tolist())


# ---- configuration ------------------------------------------------------------------------------
BASE = ["--network", "LeNet", "--dataset", "MNIST", "--device", "cpu", "--compress", "sketch"]


def test_defaults_and_describe():
    c = ewdml.parse_args(BASE)
    assert (c.sketch_rows, c.sketch_width, c.hip_graph, c.error_feedback) == (3, 2.0, "split",
                                                                              True)
    c = ewdml.parse_args(BASE + ["--sketch-rows", "5", "--sketch-width", "0.5"])
    assert (c.sketch_rows, c.sketch_width) == (5, 0.5)
    assert make_codec("sketch").describe() == "sketch-r3"
    assert make_codec("sketch", rows=1, width=1.0).describe() == "sketch-r1"
    for kw in (dict(rows=2), dict(rows=7), dict(width=0.0), dict(width=-1.0)):
        with pytest.raises(ValueError, match="sketch"):
            make_codec("sketch", **kw)
    with pytest.raises(ValueError, match="sketch codec"):
        make_codec("topk", rows=3)
    with pytest.raises(ValueError, match="bound by its own exchange"):
        make_codec("sketch").bind([], "cpu")


@pytest.mark.parametrize("extra,why", [
    (["--topology", "ps"], "--compress sketch sums its tables by all-reduce"),
    (["--topology", "sharded"], "--compress sketch sums its tables by all-reduce"),
    (["--topology", "twostage"], "--topology twostage is the sign codec's exchange"),
    (["--sync-every", "4"], "--compress sketch exchanges every step"),
    (["--select-best"], "--compress sketch sums all workers' sketches"),
    (["--predivide", "2"], "--compress sketch averages the summed values with 1/N"),
    (["--pull-compress", "qsgd"], "--compress sketch has no parameter-server form"),
    (["--optimizer", "onebit_adam", "--onebit-warmup-steps", "2"],
     "--compress sketch is not the sign codec"),
    (["--optimizer", "onebit_lamb", "--onebit-warmup-steps", "2"], "it needs --compress sign"),
    (["--sign-rotate", "hadamard"], "it needs --compress sign"),
    (["--ef-mode", "plain"], "--compress sketch keeps a plain residual"),
    (["--ef-mode", "ef21"], "--compress sketch keeps a plain residual"),
    (["--no-error-feedback"], "--compress sketch sends only the heavy coordinates"),
    (["--hip-graph", "full"], "--compress sketch issues its two all-reduces"),
    (["--hip-graph", "segmented"], "--compress sketch issues its two all-reduces"),
    (["--sketch-rows", "2"], "--sketch-rows must be 1, 3 or 5"),
    (["--sketch-width", "0"], "--sketch-width must be > 0"),
])
def test_refusals_give_their_reason(extra, why):
    with pytest.raises(ValueError, match=why):
        ewdml.parse_args(BASE + extra)


@pytest.mark.parametrize("flag", [["--sketch-rows", "3"], ["--sketch-width", "2"]])
def test_stray_sketch_flags_are_refused(flag):
    with pytest.raises(ValueError, match="belongs to --compress sketch"):
        ewdml.parse_args(["--network", "LeNet", "--device", "cpu", "--compress", "topk"] + flag)


def test_distributed_optimizer_refuses_the_sketch():
    from ewdml.parallel import horovod as hvd

    codec = hvd.Compression.sketch(5, 1.0)
    assert (codec.kind, codec.rows, codec.width) == ("sketch", 5, 1.0)
    model = torch.nn.Linear(4, 2)
    with pytest.raises(ValueError, match="two dependent all-reduces"):
        hvd.DistributedOptimizer(torch.optim.SGD(model.parameters(), lr=0.1),
                                 compression=codec)


def test_byte_formulas():
    """payload = 4 (R W + K + dense elements); each ring all-reduce moves 2 (N - 1) / N of its
    part, whatever N is; the all-gather topk receives (N - 1) payloads of about 6 K bytes."""
    sp, lay, sim = S.make_plans(3, 2.0)
    K = sum(k for k, d in zip(sp.plan.ks, sp.dense) if not d)
    assert (sp.K, sp.dense_elems, sp.W) == (K, 41, CHUNK * -(-2 * K // CHUNK))
    assert 4 * sp.payload_floats == 4 * (3 * sp.W + K + 41) == sim.payload_bytes()
    out = S.run_rank(0, 1, 1)  # a world of one: nothing on the wire
    assert out["stats"] == (4 * sum(out["floats"]), 0, 0, 2 * out["buckets"])
    # the defaults against topk's all-gather at the same k: about equal at N = 8
    R, F = 3, 2.0
    sketch8 = 2 * 7 / 8 * 4 * (R * F * K + K)
    topk8 = 7 * 6 * K
    assert 0.6 < sketch8 / topk8 < 1.4
