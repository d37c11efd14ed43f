"""Lion and Distributed Lion's 1-bit vote on the CPU: the torch oracle (compress/oracle.py
lion_apply / encode_vote / vote_apply), the ``vote`` payload layout, ``FlatLion`` and the vote
codec in a world of one, and the command line."""
import numpy as np
import pytest
import torch

import ewdml
from ewdml.compress import make_codec, oracle
from ewdml.compress.plan import CHUNK, BucketPlan, Layout

NUMELS = [1, 31, 33, 8191, 8192, 8193, 2 * 8192 + 5]

BASE = ["--network", "LeNet", "--dataset", "MNIST", "--batch-size", "16", "--synthetic-size",
        "256", "--eval-freq", "0", "--quiet", "--device", "cpu", "--lr", "0.0001",
        "--log-interval", "1000"]
VOTE = BASE + ["--compress", "vote", "--optimizer", "lion"]


def _plan(numels):
    offs, o = [], 0
    for n in numels:
        offs.append(o)
        o += (n + 63) // 64 * 64
    return BucketPlan(numels, offs, 1.0, 0, o)


def _rand(plan, seed, scale=1.0):
    """Random values without exact zeros at the tensors' positions, 0 between them."""
    g = torch.zeros(plan.length)
    gen = torch.Generator().manual_seed(seed)
    for off, n in zip(plan.offsets, plan.numels):
        v = torch.randn(n, generator=gen) * scale
        g[off:off + n] = torch.where(v == 0, torch.full_like(v, 0.5), v)
    return g


def _bits(pay, plan, lay):
    """bool [C, CHUNK] of a vote payload."""
    C = plan.num_chunks
    w = pay[lay.codes:lay.codes + 1024 * C].view(torch.int32).to(torch.int64)
    return ((w[:, None] >> torch.arange(32)) & 1).reshape(C, CHUNK).bool()


def _same(a, b):
    return torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


@pytest.mark.parametrize("wd", [0.0, 0.1])
def test_lion_apply_equals_an_independent_lion(wd):
    """A few-line Lion in fp32 tensor arithmetic (no oracle helper), exact equality."""
    gen = torch.Generator().manual_seed(3)
    n = 10007
    p, m, g = (torch.randn(n, generator=gen) for _ in range(3))
    assert bool((g != 0).all()) and bool((m != 0).all())
    lr, b1, b2 = 1e-3, 0.9, 0.99
    t = lambda v: torch.tensor(v, dtype=torch.float32)  # noqa: E731
    pr, mr = p.clone(), m.clone()
    for _ in range(3):
        c = mr * t(b1) + (t(1.0) - t(b1)) * g
        u = torch.sign(c)
        pr = pr - t(lr) * (u + t(wd) * pr) if wd else pr - t(lr) * u
        mr = mr * t(b2) + (t(1.0) - t(b2)) * g
        oracle.lion_apply(p, m, g, lr, b1, b2, wd)
        assert _same(p, pr) and _same(m, mr)


def test_lion_apply_zero_and_nan_give_no_sign_step():
    p = torch.tensor([1.0, 2.0, 3.0, 4.0])
    m = torch.tensor([0.0, -0.0, float("nan"), 1.0])
    g = torch.tensor([0.0, -0.0, 1.0, -5.0])
    oracle.lion_apply(p, m, g, 0.5, 0.5, 0.5, 0.0)
    assert p.tolist() == [1.0, 2.0, 3.0, 4.5]  # c = 0, -0, NaN: u = 0; c = -2: u = -1


@pytest.mark.parametrize("rank", [0, 1])
@pytest.mark.parametrize("step", [1, 2])
def test_encode_vote_planted_bits(step, rank):
    """Exact zeros in both g and m at even and odd indices, -0.0 and one NaN: the bits by the
    closed form (c < 0) | ((c == 0) & ((i + step + rank) & 1))."""
    plan = _plan([8192 + 40, 33])
    lay = Layout.build("vote", plan)
    g, m = _rand(plan, 1), _rand(plan, 2)
    o1 = plan.offsets[1]
    zeros = [0, 1, 6, 7, 8191, 8192, 8193, 8192 + 39, o1, o1 + 1, o1 + 32]
    for z in zeros:
        g[z] = 0.0
        m[z] = 0.0
    g[10], m[10] = -0.0, -0.0  # c = -0.0 == 0: dithered like +0
    g[11], m[11] = -0.0, 0.0
    g[20] = float("nan")
    g[21], m[21] = 0.0, -3.0  # a zero gradient under a negative momentum is a plain -1
    b1, b2 = 0.9, 0.99
    m0 = m.clone()
    pay = oracle.encode_vote(g, plan, lay, m, b1, b2, step, rank)
    assert pay.dtype == torch.uint8 and pay.numel() == lay.nbytes == 1024 * plan.num_chunks
    bits = _bits(pay, plan, lay)
    f32 = np.float32
    c = (m0.numpy() * f32(b1) + (f32(1) - f32(b1)) * g.numpy()).astype(np.float32)
    for ci, (t, s, ln) in enumerate(zip(plan.chunk_tensor, plan.chunk_start, plan.chunk_len)):
        i = np.arange(ln)
        cc = c[s:s + ln]
        want = (cc < 0) | ((cc == 0) & (((i + step + rank) & 1) == 1))
        assert np.array_equal(bits[ci, :ln].numpy(), want), ci
        assert not bits[ci, ln:].any()  # bits past the chunk's length
    par = (step + rank) & 1
    # chunk 0 / index i: bit = parity of i + step + rank at the planted zeros
    for z in (0, 1, 6, 7, 8191, 10, 11):
        assert bool(bits[0, z]) == bool((z + par) & 1)
    for z in (8192, 8193, 8192 + 39):  # chunk 1 of tensor 0: chunk-local index
        assert bool(bits[1, z - 8192]) == bool((z - 8192 + par) & 1)
    for z in (0, 1, 32):  # tensor 1 starts its own chunk
        assert bool(bits[2, z]) == bool((z + par) & 1)
    assert not bool(bits[0, 20]) and bool(bits[0, 21])  # NaN: +1; -2.7: -1
    # the momentum moved everywhere inside the tensors and nowhere between them
    want_m = (m0.numpy() * f32(b2) + (f32(1) - f32(b2)) * g.numpy()).astype(np.float32)
    inside = torch.zeros(plan.length, dtype=torch.bool)
    for off, n in zip(plan.offsets, plan.numels):
        inside[off:off + n] = True
    ok = ~torch.isnan(g) & inside
    assert _same(m[ok], torch.from_numpy(want_m)[ok]) and torch.isnan(m[20])
    assert _same(m[~inside], m0[~inside])


def test_vote_layout_and_padding_bits():
    plan = _plan(NUMELS)
    lay = Layout.build("vote", plan)
    C = plan.num_chunks
    assert C == 1 + 1 + 1 + 1 + 1 + 2 + 3
    assert (lay.kind, lay.codes, lay.nbytes) == ("vote", 0, 1024 * C)
    sign = Layout.build("sign", plan)
    assert sign.nbytes - sign.codes == lay.nbytes  # the sign layout minus its scales section
    g = -_rand(plan, 5).abs()  # every element votes -1: every valid bit is set
    pay = oracle.encode_vote(g, plan, lay, torch.zeros(plan.length), 0.9, 0.99, 1, 0)
    bits = _bits(pay, plan, lay)
    for ci, ln in enumerate(plan.chunk_len):
        assert bits[ci, :ln].all() and not bits[ci, ln:].any()
    with pytest.raises(ValueError):
        oracle.encode_vote(g, plan, sign, torch.zeros(plan.length), 0.9, 0.99, 1, 0)


def _votes(plan, lay, N, seed=40):
    return torch.stack([oracle.encode_vote(_rand(plan, seed + r), plan, lay,
                                           torch.zeros(plan.length), 0.0, 0.0, 1, r)
                        for r in range(N)])


def _applied(recv, plan, lay, aggregate, wd=0.0, lr=0.25):
    p0 = torch.round(_rand(plan, 9) * 8) / 8  # multiples of 1/8: p0 - lr * d is exact
    p = p0.clone()
    oracle.vote_apply(recv, plan, lay, p, lr, wd, aggregate, 1.0 / recv.shape[0])
    return p0, p


def test_vote_apply_aggregation():
    plan = _plan([500, 8192 + 3, 31])
    lay = Layout.build("vote", plan)
    inside = torch.zeros(plan.length, dtype=torch.bool)
    for off, n in zip(plan.offsets, plan.numels):
        inside[off:off + n] = True
    lr = 0.25  # a power of two: lr * d is exact and d = (p0 - p) / lr
    # N = 2: ties, d == 0 there, and majority == average on {-1, 0, 1}
    recv = _votes(plan, lay, 2)
    p0, pm = _applied(recv, plan, lay, "majority")
    _, pa = _applied(recv, plan, lay, "average")
    d = (p0 - pm) / lr
    assert set(d[inside].tolist()) == {-1.0, 0.0, 1.0}
    s = oracle.vote_counts(recv, plan, lay)
    assert bool((s == 0).any())
    assert _same(pm, pa)
    assert _same(pm[~inside], p0[~inside])  # positions between tensors are not touched
    # N = 3 never ties
    recv = _votes(plan, lay, 3)
    p0, pm = _applied(recv, plan, lay, "majority")
    assert set(((p0 - pm) / lr)[inside].tolist()) == {-1.0, 1.0}
    # N = 4, average: multiples of 1/2
    recv = _votes(plan, lay, 4)
    p0, pa = _applied(recv, plan, lay, "average")
    assert set(((p0 - pa) / lr)[inside].tolist()) == {-1.0, -0.5, 0.0, 0.5, 1.0}
    # weight decay enters as p - lr * (d + wd * p)
    p0, pw = _applied(recv, plan, lay, "average", wd=0.1)
    dd = ((p0 - pa) / lr)
    want = p0 - (dd + p0 * float(np.float32(0.1))) * lr
    assert _same(pw[inside], want[inside])
    with pytest.raises(ValueError):
        oracle.vote_apply(recv, plan, lay, p0, lr, 0.0, "median", 0.25)


@pytest.mark.parametrize("N", [2, 3, 5])
def test_zero_betas_are_signsgd_with_majority_vote(N):
    plan = _plan([700, 8192 + 1])
    lay = Layout.build("vote", plan)
    grads = [_rand(plan, 70 + r) for r in range(N)]
    moms = [_rand(plan, 90 + r) for r in range(N)]  # ignored: beta1 = 0; replaced: beta2 = 0
    recv = torch.stack([oracle.encode_vote(g, plan, lay, m, 0.0, 0.0, 3, r)
                        for r, (g, m) in enumerate(zip(grads, moms))])
    p0 = _rand(plan, 9)
    p = p0.clone()
    oracle.vote_apply(recv, plan, lay, p, 0.125, 0.0, "majority", 1.0 / N)
    want = p0 - 0.125 * torch.sign(sum(torch.sign(g) for g in grads))
    assert _same(p, want)
    for g, m in zip(grads, moms):
        assert _same(m, g)  # m = 0 * m + 1 * g


@pytest.mark.parametrize("aggregate", ["majority", "average"])
@pytest.mark.parametrize("wd", [0.0, 0.1])
def test_world_of_one_vote_is_dense_lion(wd, aggregate):
    """Encode, then apply at N = 1: bitwise the dense step on inputs without an exact zero c."""
    plan = _plan(NUMELS)
    lay = Layout.build("vote", plan)
    p, m = _rand(plan, 1), _rand(plan, 2)
    pd, md = p.clone(), m.clone()
    lr, b1, b2 = 3e-4, 0.9, 0.99
    for step in range(1, 4):
        g = _rand(plan, 10 + step)
        pay = oracle.encode_vote(g, plan, lay, m, b1, b2, step, 0)
        oracle.vote_apply(pay[None], plan, lay, p, lr, wd, aggregate, 1.0)
        for off, n in zip(plan.offsets, plan.numels):
            sl = slice(off, off + n)
            oracle.lion_apply(pd[sl], md[sl], g[sl], lr, b1, b2, wd)
        assert _same(p, pd) and _same(m, md)


def test_zero_gradient_parameter_does_not_drift_at_world_one():
    """The dither: an identically zero gradient votes +1, -1, +1, ... and cancels over two steps."""
    plan = _plan([64])
    lay = Layout.build("vote", plan)
    p = torch.ones(plan.length)
    m = torch.zeros(plan.length)
    for step in range(1, 5):
        pay = oracle.encode_vote(torch.zeros(plan.length), plan, lay, m, 0.9, 0.99, step, 0)
        oracle.vote_apply(pay[None], plan, lay, p, 0.25, 0.0, "majority", 1.0)
    assert torch.equal(p, torch.ones(plan.length))


def test_flat_lion_and_vote_exchange_in_a_world_of_one():
    """FlatLion's dense step and the vote exchange (GradientExchange, N = 1) on the same
    gradients: the same parameters and momentum, bit for bit; state dict round trip."""
    from ewdml.optim.flat import FlatLion, make_optimizer
    from ewdml.parallel.comm import Comm
    from ewdml.parallel.engine import GradientExchange
    from ewdml.parallel.flat import FlatModel

    def flat():
        gen = torch.Generator().manual_seed(7)
        return FlatModel([torch.nn.Parameter(torch.randn(n, generator=gen))
                          for n in (500, 20, 8193, 1)], bucket_bytes=16 << 10, reverse=False)

    fa, fb = flat(), flat()
    oa = make_optimizer("lion", fa, lr=1e-3, betas=(0.9, 0.99), weight_decay=0.1)
    ob = FlatLion(fb, lr=1e-3, weight_decay=0.1)
    assert isinstance(oa, FlatLion) and oa.lion and not oa.fusable and oa.betas == (0.9, 0.99)
    assert set(oa.hparams()) >= {"lr", "betas", "weight_decay", "step_t", "lr_t"}
    codec = make_codec("vote", aggregate="majority")
    assert codec.describe() == "vote1b" and not codec.allreduce
    ex = GradientExchange(fb, Comm(), codec, ob, overlap=False, side_stream=False)
    assert ex.vote and ex.resid is None and ex.vel is None and len(fb.buckets) > 1
    assert [codec.payload_bytes(b.index) for b in fb.buckets] == \
        [1024 * b.plan.num_chunks for b in fb.buckets]
    gen = torch.Generator().manual_seed(11)
    for _ in range(3):
        g = torch.randn(fa.numel, generator=gen)
        oa.step(g)
        fb.grad.copy_(g)
        ex.begin()
        ex.finish()
    assert oa.steps == ob.steps == 3
    inside = torch.zeros(fa.numel, dtype=torch.bool)
    for p, off in zip(fa.params, fa.offsets):
        inside[off:off + p.numel()] = True
    assert _same(fa.data[inside], fb.data[inside]) and _same(oa.exp_avg[inside], ob.exp_avg[inside])
    sd = oa.state_dict()
    assert sd["kind"] == "lion" and set(sd) == {"kind", "exp_avg", "steps", "lr"}
    oc = FlatLion(flat(), lr=5.0)
    oc.load_state_dict(sd)
    assert oc.steps == 3 and oc.lr == 1e-3 and torch.equal(oc.exp_avg, oa.exp_avg)
    ex.close()
    with pytest.raises(ValueError, match="betas"):
        FlatLion(flat(), betas=(0.9, 1.0))


def test_vote_codec_refuses_other_optimizers_and_plain_encode():
    from ewdml.optim.flat import FlatAdam, FlatLion, FlatSGD
    from ewdml.parallel.comm import Comm
    from ewdml.parallel.engine import GradientExchange
    from ewdml.parallel.flat import FlatModel

    flat = FlatModel([torch.nn.Parameter(torch.randn(100))], bucket_bytes=1 << 20, reverse=False)
    for opt in (FlatSGD(flat, lr=0.1), FlatAdam(flat)):
        with pytest.raises(ValueError, match="no magnitudes"):
            GradientExchange(flat, Comm(), make_codec("vote"), opt, overlap=False)
    with pytest.raises(ValueError, match="error feedback"):
        GradientExchange(flat, Comm(), make_codec("vote"), FlatLion(flat), overlap=False,
                         error_feedback=True)
    with pytest.raises(ValueError, match="predivide"):
        GradientExchange(flat, Comm(), make_codec("vote"), FlatLion(flat), overlap=False,
                         predivide=2.0)
    with pytest.raises(ValueError):
        make_codec("vote", aggregate="median")
    with pytest.raises(ValueError):
        make_codec("sign", aggregate="average")
    ex = GradientExchange(flat, Comm(), make_codec("vote", aggregate="average"), FlatLion(flat),
                          overlap=False)
    with pytest.raises(ValueError, match="encode_vote"):
        ex.codec.encode(0, flat.grad, ex.payload[0], 0, 0)
    with pytest.raises(ValueError, match="no magnitudes"):
        ex.codec.decode(0, ex.recv[0].view(1, -1), flat.grad, 1.0)
    ex.close()


def test_plan_graph_mode_treats_vote_as_the_sign_family():
    from ewdml.parallel.engine import plan_graph_mode

    kw = dict(grad_numel=9_231_114, model="VGG11")
    for world in (1, 8):
        a = plan_graph_mode(world, "rccl-stream", "sign", **kw)
        b = plan_graph_mode(world, "rccl-stream", "vote", **kw)
        assert a == b and b["wire_bytes"] == int((world - 1) * kw["grad_numel"] / 8)


# ---- command line ---------------------------------------------------------------------------------
def test_cli_defaults():
    c = ewdml.parse_args(VOTE)
    assert c.optimizer == "lion" and c.compress == "vote"
    assert c.lion_betas == (0.9, 0.99) and c.vote_aggregate == "majority"
    assert c.error_feedback is False
    assert c.resolved().lion_betas == (0.9, 0.99)  # resolving twice is harmless
    c = ewdml.parse_args(VOTE + ["--lion-betas", "0,0", "--vote-aggregate", "average",
                                 "--no-error-feedback", "--clip-grad-norm", "1.0"])
    assert c.lion_betas == (0.0, 0.0) and c.vote_aggregate == "average"
    assert c.clip_grad_norm == 1.0 and c.error_feedback is False
    # plain Lion on the decoded averaged gradient of any other codec, wherever adam runs
    for extra in (["--compress", "none"], ["--compress", "topk_qsgd"], ["--compress", "sign"],
                  ["--compress", "qsgd", "--topology", "ps"],
                  ["--compress", "topk_qsgd", "--topology", "sharded"],
                  ["--compress", "powersgd"], ["--compress", "none", "--sync-every", "4"]):
        for o in ("lion", "adam"):
            c = ewdml.parse_args(BASE + ["--optimizer", o] + extra)
            assert c.optimizer == o and c.vote_aggregate is None


@pytest.mark.parametrize("extra, reason", [
    (["--optimizer", "sgd"], "--compress vote .*--optimizer lion"),
    (["--optimizer", "adam"], "--compress vote .*--optimizer lion"),
    (["--optimizer", "lion", "--topology", "ps"], "--compress vote .*--topology ps"),
    (["--optimizer", "lion", "--topology", "sharded"], "--compress vote .*--topology sharded"),
    (["--optimizer", "lion", "--topology", "twostage"], "--compress vote .*--topology twostage"),
    (["--optimizer", "lion", "--sync-every", "2"], "--compress vote .*--sync-every"),
    (["--optimizer", "lion", "--select-best"], "--compress vote .*--select-best"),
    (["--optimizer", "lion", "--predivide", "2"], "--compress vote .*--predivide"),
    (["--optimizer", "lion", "--error-feedback"], "--compress vote .*--error-feedback"),
])
def test_cli_vote_refusals(extra, reason):
    with pytest.raises(ValueError, match=reason):
        ewdml.parse_args(BASE + ["--compress", "vote"] + extra)


@pytest.mark.parametrize("extra, reason", [
    (["--optimizer", "adam", "--lion-betas", "0.9,0.99"], "--lion-betas belongs to"),
    (["--optimizer", "lion", "--lion-betas", "0.9"], "--lion-betas takes B1,B2"),
    (["--optimizer", "lion", "--lion-betas", "0.9,1.0"], "--lion-betas takes B1,B2"),
    (["--optimizer", "lion", "--lion-betas=-0.1,0.5"], "--lion-betas takes B1,B2"),
    (["--optimizer", "lion", "--lion-betas", "a,b"], "--lion-betas takes B1,B2"),
    (["--optimizer", "lion", "--compress", "sign", "--vote-aggregate", "average"],
     "--vote-aggregate belongs to"),
])
def test_cli_flag_refusals(extra, reason):
    with pytest.raises(ValueError, match=reason):
        ewdml.parse_args(BASE + extra)


@pytest.mark.parametrize("comp", ["vote", "none", "topk_qsgd"])
def test_trainer_steps_with_lion_on_the_cpu(comp):
    """Through the trainer on the CPU at a world of one: Lion under the vote codec, dense and on a
    decoded top-k gradient; in vote mode the momentum travels in the checkpoint extras as one row
    per rank."""
    from ewdml.runtime import Trainer

    tr = Trainer(ewdml.parse_args(BASE + ["--compress", comp, "--optimizer", "lion",
                                          "--max-steps", "3"]))
    before = tr.flat.data.clone()
    for _ in range(3):
        loss, _ = tr.train_step()
        assert torch.isfinite(loss)
    assert tr.opt.steps == 3 and not torch.equal(before, tr.flat.data)
    assert float(tr.opt.exp_avg.abs().max()) > 0
    ext = tr.state_extra()
    if comp == "vote":
        assert tr.exchange.vote and tr.exchange.last.payload_bytes == sum(
            1024 * b.plan.num_chunks for b in tr.flat.buckets)
        assert ext["lion_momentum"].shape == (1, tr.flat.numel)
        assert torch.equal(ext["lion_momentum"][0], tr.opt.exp_avg)
        step = (tr.flat.data - before).abs().max()
        assert float(step) <= 3 * 1e-4 * 1.0001  # every step moves a parameter by at most lr
    else:
        assert not tr.exchange.vote and "lion_momentum" not in ext
    tr.close()
