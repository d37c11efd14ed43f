"""Two-stage sign all-reduce (``--topology twostage``) on the CPU: the owner step's oracle identity,
the slot table of the ``[N, P]`` row buffers, the lossless second quantisation, the refused flag
combinations and the three-codec-calls-per-bucket count."""
import pytest
import torch

from ewdml.compress import CHUNK, BucketPlan, Layout, TwoStagePlan, make_codec, oracle
from ewdml.parallel.sharded import shard_plans

from ..twostage_sim import make_flat, make_opt, same_bits

SIZES = [1, 31, 8192, 8193, 20000]


def _bucket(numels, start=0):
    offsets, o = [], 0
    for n in numels:
        offsets.append(o)
        o += (n + 63) // 64 * 64
    return BucketPlan(numels, offsets, 1.0, start, o)


def _ts(numels, n):
    plan = _bucket(numels)
    return TwoStagePlan(plan, shard_plans(plan, n, 0))


def test_reduce_encode_is_decode_then_encode():
    plan = _bucket([20000, 31])
    lay = Layout.build("sign", plan)
    gen = torch.Generator().manual_seed(0)
    for n in (1, 3):
        recv = torch.zeros((n, lay.nbytes + 48), dtype=torch.uint8)  # rows wider than the payload
        for r in range(n):
            recv[r, :lay.nbytes] = oracle.encode_sign(
                torch.randn(plan.length, generator=gen), plan, lay, None)
        sres = torch.randn(plan.length, generator=gen) * 0.01
        a, b = sres.clone(), sres.clone()
        got = oracle.sign_reduce_encode(recv, plan, lay, 1.0 / n, a)
        mean = oracle.decode_sum(recv[:, :lay.nbytes].contiguous(), plan, lay, 0, 1.0 / n)
        want = oracle.encode_sign(mean, plan, lay, b)
        assert torch.equal(got, want)
        assert same_bits(a, b) and not same_bits(a, sres)


@pytest.mark.parametrize("n", [1, 2, 3, 8])
def test_slot_table(n):
    ts = _ts(SIZES, n)
    plan = ts.plan
    assert plan.num_chunks == len(ts.slots) and plan.numel == sum(SIZES)
    # a tensor crossing a cut is two segments, each chunked from its own start
    assert all(s0 % CHUNK == 0 for s0, _, _, _, _ in ts.shards)
    used = torch.zeros(n * ts.P, dtype=torch.int32)
    c = 0
    for r, (s0, ln, sp, lay, c0) in enumerate(ts.shards):
        if sp is None:
            continue
        assert c0 == c and lay.nbytes <= ts.P
        for j in range(sp.num_chunks):
            a, w = ts.slots[c]
            assert a == r * ts.P + lay.scales + 4 * j  # the shard's own layout inside row r
            assert w == r * ts.P + lay.codes + 1024 * j and w % 16 == 0
            assert w + 1024 <= r * ts.P + lay.nbytes
            assert plan.chunk_start[c] == s0 + sp.chunk_start[j]
            assert plan.chunk_len[c] == sp.chunk_len[j]
            used[a:a + 4] += 1
            used[w:w + 1024] += 1
            c += 1
    assert int(used.max()) == 1  # no two chunks overlap
    assert ts.slot_end == int(used.nonzero().max()) + 1

    # push: every byte outside the slots stays 0, and row r is shard r's payload
    codec = make_codec("sign").bind_twostage([ts], "cpu")
    gen = torch.Generator().manual_seed(n)
    g = torch.randn(plan.length, generator=gen)
    resid = torch.zeros(plan.length)
    rows = torch.zeros((n, ts.P), dtype=torch.uint8)
    codec.ts_encode(0, g, rows, resid)
    assert int(rows.view(-1)[used == 0].abs().max() if (used == 0).any() else 0) == 0
    for r, (s0, ln, sp, lay, _) in enumerate(ts.shards):
        if sp is None:
            assert int(rows[r].abs().max()) == 0  # an empty shard's row is a zero row
            continue
        want = oracle.encode_sign(g[s0:s0 + ln], sp, lay, torch.zeros(ln))
        assert torch.equal(rows[r, :lay.nbytes], want)
    # pull: reading every chunk through its slot is the per-shard decode
    flat = rows.view(-1)
    got = torch.zeros(plan.length)
    sh = torch.arange(32)
    for c, (a, w) in enumerate(ts.slots):
        scale = flat[a:a + 4].view(torch.float32)
        words = flat[w:w + 1024].view(torch.int32).to(torch.int64)
        neg = ((words[:, None] >> sh) & 1).flatten().bool()[:plan.chunk_len[c]]
        got[plan.chunk_start[c]:plan.chunk_start[c] + plan.chunk_len[c]] = \
            torch.where(neg, -scale, scale)
    assert same_bits(got, codec._ts_decoded(0, rows))


def test_too_many_segments_raise():
    with pytest.raises(ValueError, match="128"):
        _ts([64] * 129, 2)


def test_second_quantisation_lossless_on_constant_magnitude_chunks():
    plan = _bucket([20000, 3])
    lay = Layout.build("sign", plan)
    gen = torch.Generator().manual_seed(3)
    g = torch.zeros(plan.length)
    for c, (s, ln) in enumerate(zip(plan.chunk_start, plan.chunk_len)):
        sign = torch.randint(0, 2, (ln,), generator=gen).float() * 2 - 1
        g[s:s + ln] = sign * 2.0 ** (c - 3)
    pay = oracle.encode_sign(g, plan, lay, torch.zeros(plan.length))
    sres = torch.zeros(plan.length)
    again = oracle.sign_reduce_encode(pay[None], plan, lay, 1.0, sres)
    assert torch.equal(again, pay)
    assert int(sres.view(torch.int32).abs().max()) == 0


@pytest.mark.parametrize("flags,match", [
    (["--compress", "topk_qsgd"], "compress sign"),
    (["--compress", "none"], "compress sign"),
    (["--compress", "qsgd"], "compress sign"),
    (["--compress", "sign", "--no-error-feedback"], "no-error-feedback"),
    (["--compress", "sign", "--sync-every", "4"], "sync-every"),
    (["--compress", "sign", "--select-best"], "select-best"),
    (["--compress", "sign", "--predivide", "2"], "predivide"),
    (["--compress", "sign", "--hip-graph", "full"], "hip-graph full"),
    (["--compress", "sign", "--hip-graph", "segmented"], "hip-graph segmented"),
])
def test_refusals(flags, match):
    import ewdml

    with pytest.raises(ValueError, match=match) as e:
        ewdml.parse_args(["--topology", "twostage"] + flags)
    assert "twostage" in str(e.value)


def test_accepted_and_sharded_still_refused():
    import ewdml

    cfg = ewdml.parse_args(["--topology", "twostage", "--compress", "sign"])
    assert cfg.topology == "twostage" and cfg.error_feedback is True
    cfg = ewdml.parse_args(["--topology", "twostage", "--compress", "sign", "--optimizer",
                            "onebit_adam", "--onebit-warmup-steps", "3", "--hip-graph", "split"])
    assert cfg.optimizer == "onebit_adam"
    with pytest.raises(ValueError, match="twostage"):  # the refusal now points at the new topology
        ewdml.parse_args(["--topology", "sharded", "--compress", "sign"])


class _Comm:
    """World of 3 seen from rank 1, collectives stubbed: enough to count launches."""
    world, rank, kind = 3, 1, "stub"

    def all_to_all(self, out, inp):
        out.copy_(inp)

    def all_gather(self, out, inp):
        pass


@pytest.mark.parametrize("kind", ["sgd", "onebit"])
def test_three_codec_calls_per_bucket_per_step(kind):
    from ewdml.parallel.twostage import TwoStageSignExchange

    flat = make_flat()
    opt = make_opt(flat, kind)
    if kind == "onebit":
        opt.steps = opt.freeze_step
        opt.exp_avg_sq.fill_(1.0)
    ex = TwoStageSignExchange(flat, _Comm(), make_codec("sign"), opt)
    assert len(flat.buckets) == 2
    assert all(t.shards[1][2] is not None for t in ex.ts)  # rank 1 owns a shard of each
    calls = []
    for name in ("ts_encode", "ts_reduce_encode", "ts_decode_apply_sgd",
                 "ts_decode_apply_onebit"):
        def wrap(*a, _f=getattr(ex.codec, name), _n=name, **k):
            calls.append((_n, a[0]))
            return _f(*a, **k)
        setattr(ex.codec, name, wrap)
    pull = "ts_decode_apply_onebit" if kind == "onebit" else "ts_decode_apply_sgd"
    for step in range(2):
        del calls[:]
        flat.grad.copy_(torch.randn(flat.numel))
        ex.begin()
        ex.finish()
        for b in range(2):
            assert [n for n, bi in calls if bi == b] == ["ts_encode", "ts_reduce_encode", pull]
        assert len(calls) == 3 * len(flat.buckets)
    assert float(ex.resid.abs().max()) > 0 and float(ex.sresid.abs().max()) > 0
