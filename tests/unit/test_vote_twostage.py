"""The two-stage vote (``--compress vote --vote-exchange twostage``) on the CPU: the owner step's
oracle against a plain loop, the ``vote`` slot table of the ``[N, P]`` row buffers, a world of N
exchanges in one process against the all-gather vote, the flags, and the launch count."""
import threading

import pytest
import torch

from ewdml.compress import CHUNK, BucketPlan, Layout, TwoStagePlan, make_codec, oracle
from ewdml.parallel.sharded import shard_plans

from ..twostage_sim import BUCKET_BYTES, grad_of, same_bits

# the last tensor's gradient is identically zero: its votes are the dither alone
NUMELS = [2 * 8192 + 5, 3, 8191, 8193, 70, 100]
ZERO_TENSOR = 5
LR, WD, BETAS = 2.0 ** -6, 0.1, (0.9, 0.99)
STEPS = 5


def _bucket(numels, start=0):
    offsets, o = [], 0
    for n in numels:
        offsets.append(o)
        o += (n + 63) // 64 * 64
    return BucketPlan(numels, offsets, 1.0, start, o)


def _unpack(pay, C):
    """bool [C, CHUNK] of a vote payload's first C chunks."""
    w = pay[:1024 * C].view(torch.int32).to(torch.int64)
    return ((w[:, None] >> torch.arange(32)) & 1).reshape(C, CHUNK).bool()


# ---- the owner step ---------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 2, 3, 4])
def test_vote_reduce_against_a_plain_loop(n):
    plan = _bucket([70, 8193])  # 3 chunks of 70, 8192 and 1 elements
    lay = Layout.build("vote", plan)
    C = plan.num_chunks
    gen = torch.Generator().manual_seed(10 + n)
    valid = torch.arange(CHUNK)[None, :] < torch.tensor(plan.chunk_len)[:, None]
    bits = (torch.randint(0, 2, (n, C, CHUNK), generator=gen).bool()) & valid
    if n % 2 == 0:  # forced ties: the second half of the rows votes against the first
        bits[n // 2:, :, :4096] = ~bits[:n // 2, :, :4096] & valid[:, :4096]
    bits[:, 1, 100:164] = True  # all-set words
    bits[:, 1, 200:264] = False  # all-clear words
    sh = torch.arange(32, dtype=torch.int64)
    words = (bits.reshape(n, C, CHUNK // 32, 32).to(torch.int64) << sh).sum(-1)
    words = (((words + (1 << 31)) % (1 << 32)) - (1 << 31)).to(torch.int32)
    recv = torch.full((n, lay.nbytes + 32), 0xA5, dtype=torch.uint8)  # rows wider than the payload
    recv[:, :lay.nbytes] = words.reshape(n, -1).view(torch.uint8)
    for owner in range(n):
        got = oracle.vote_reduce(recv, plan, lay, owner)
        assert got.dtype == torch.uint8 and got.numel() == lay.nbytes
        got = _unpack(got, C).tolist()
        b = bits.tolist()
        ties = 0
        for c in range(C):
            for i in range(CHUNK):
                s = n - 2 * sum(b[r][c][i] for r in range(n))
                want = s < 0 or (s == 0 and b[owner][c][i])
                ties += s == 0
                assert got[c][i] == want, (owner, c, i)
                if i >= plan.chunk_len[c]:
                    assert not got[c][i]  # padding bits stay 0
        assert (ties > 0) == (n % 2 == 0)
    with pytest.raises(ValueError, match="owner row"):
        oracle.vote_reduce(recv, plan, lay, n)
    with pytest.raises(ValueError, match="sign"):
        oracle.vote_reduce(recv, plan, Layout.build("sign", plan), 0)


# ---- the plan ---------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 2, 3, 8])
def test_vote_slot_table(n):
    plan = _bucket([1, 31, 8192, 8193, 20000])
    ts = TwoStagePlan(plan, shard_plans(plan, n, 0), kind="vote")
    assert ts.kind == "vote"
    assert ts.P == 1024 * max(sp.num_chunks for _, _, sp, _, _ in ts.shards if sp is not None)
    want = []
    for r, (s0, ln, sp, lay, c0) in enumerate(ts.shards):
        if sp is None:
            assert lay is None
            continue
        assert c0 == len(want)
        assert (lay.kind, lay.codes, lay.nbytes) == ("vote", 0, 1024 * sp.num_chunks)
        want += [(r * ts.P + 1024 * j,) * 2 for j in range(sp.num_chunks)]
    assert ts.slots == want and len(want) == ts.plan.num_chunks
    assert ts.slot_end == max(w for _, w in want) + 1024 <= n * ts.P
    assert tuple(ts.slot_table("cpu").shape) == (len(want), 2)
    with pytest.raises(ValueError, match="sign or the vote"):
        TwoStagePlan(plan, shard_plans(plan, n, 0), kind="topk")


def test_default_kind_is_the_sign_plan_unchanged():
    plan = _bucket([1, 31, 8192, 8193, 20000])
    for n in (1, 3):
        a = TwoStagePlan(plan, shard_plans(plan, n, 0))
        b = TwoStagePlan(plan, shard_plans(plan, n, 0), kind="sign")
        lays = [Layout.build("sign", sp) for _, _, sp in shard_plans(plan, n, 0)]
        assert a.P == b.P == max(lay.nbytes for lay in lays)
        slots = [(r * a.P + 4 * j, r * a.P + lay.codes + 1024 * j)
                 for r, lay in enumerate(lays) for j in range((lay.nbytes - lay.codes) // 1024)]
        assert a.slots == b.slots == slots
        assert a.slot_end == b.slot_end == slots[-1][1] + 1024
        assert [x[3] for x in a.shards] == lays and a.max_shard == b.max_shard


# ---- a world in one process ---------------------------------------------------------------------
class _World:
    """N ranks as N threads: the collectives meet at a barrier and copy rows."""

    def __init__(self, n):
        self.n = n
        self.bar = threading.Barrier(n)
        self.post = [None] * n

    def comm(self, rank):
        return _ThreadComm(self, rank)


class _ThreadComm:
    kind = "threads"

    def __init__(self, w, rank):
        self.w, self.world, self.rank = w, w.n, rank

    def all_to_all(self, out, inp):
        w = self.w
        w.post[self.rank] = inp
        w.bar.wait()
        for j in range(w.n):
            out[j].copy_(w.post[j][self.rank])
        w.bar.wait()

    def all_gather(self, out, inp):
        w = self.w
        w.post[self.rank] = inp.clone()
        w.bar.wait()
        out.view(w.n, -1).copy_(torch.stack(w.post))
        w.bar.wait()


def _flat():
    from ewdml.parallel.flat import FlatModel

    gen = torch.Generator().manual_seed(7)
    params = [torch.nn.Parameter(torch.randn(n, generator=gen) * 0.1) for n in NUMELS]
    return FlatModel(params, bucket_bytes=BUCKET_BYTES, reverse=False)


def _grad(flat, step, rank):
    g = grad_of(step, rank, flat.numel)
    g[flat.offsets[ZERO_TENSOR]:flat.offsets[ZERO_TENSOR] + NUMELS[ZERO_TENSOR]] = 0
    return g


def _allgather_step(flat, p, moms, grads, step):
    """One step of the all-gather majority vote straight from the oracle on ``p`` (updated in
    place; ``moms`` too).  Returns per bucket (s, owner-independent row bits [N, C, CHUNK])."""
    N = len(moms)
    out = []
    for b in flat.buckets:
        lay = Layout.build("vote", b.plan)
        sl = slice(b.start, b.start + b.length)
        rows = torch.stack([oracle.encode_vote(grads[r][sl], b.plan, lay, moms[r][sl], *BETAS,
                                               step, r) for r in range(N)])
        out.append((oracle.vote_counts(rows, b.plan, lay),
                    torch.stack([_unpack(rows[r], b.plan.num_chunks) for r in range(N)])))
        oracle.vote_apply(rows, b.plan, lay, p[sl], LR, WD, "majority", 1.0 / N)
    return out


@pytest.mark.parametrize("n", [1, 2, 3, 4])
def test_world_simulation_against_the_allgather_vote(n):
    from ewdml.optim.flat import FlatLion
    from ewdml.parallel.twostage import TwoStageVoteExchange

    world = _World(n)
    flats = [_flat() for _ in range(n)]
    assert len(flats[0].buckets) > 1
    opts = [FlatLion(f, lr=LR, betas=BETAS, weight_decay=WD) for f in flats]
    exs = [TwoStageVoteExchange(f, world.comm(r), make_codec("vote"), o)
           for r, (f, o) in enumerate(zip(flats, opts))]
    assert all(ex.vote and not hasattr(ex, "resid") for ex in exs)
    ref = _flat()  # the all-gather vote: common parameters, every rank's own momentum
    p_ag = ref.data.clone()
    m_ag = [torch.zeros(ref.numel) for _ in range(n)]
    ties = 0
    for step in range(STEPS):
        grads = [_grad(ref, step, r) for r in range(n)]
        before = flats[0].data.clone()
        errs = []

        def run(r):
            try:
                flats[r].grad.copy_(grads[r])
                exs[r].begin()
                exs[r].finish()
            except BaseException as e:  # noqa: BLE001 - reported by the main thread
                errs.append(e)
                world.bar.abort()

        threads = [threading.Thread(target=run, args=(r,)) for r in range(n)]
        for t in threads:
            t.start()
        for t in threads:
            t.join()
        assert not errs, errs
        votes = _allgather_step(ref, p_ag, m_ag, grads, step + 1)
        for r in range(n):  # replicas identical; momenta are the all-gather vote's, bitwise
            assert same_bits(flats[r].data, flats[0].data), (step, r)
            assert same_bits(opts[r].exp_avg, m_ag[r]), (step, r)
        # the step every replica took: sign(s), and the owner's own vote where s == 0
        want = before.clone()
        for b, (s, bits) in zip(ref.buckets, votes):
            pos, valid, _ = oracle._sign_gather(b.plan, "cpu")
            owner = torch.zeros(b.length, dtype=torch.int64)
            for r, (s0, ln, _) in enumerate(shard_plans(b.plan, n, b.start)):
                owner[s0:s0 + ln] = r
            own = torch.gather(bits, 0, owner[pos][None])[0]
            d = torch.where(s != 0, torch.sign(s), 1 - 2 * own.to(torch.int32)).to(torch.float32)
            ties += int(((s == 0) & valid).sum())
            at = pos[valid] + b.start
            want[at] = oracle._lion_step(before[at], d[valid], LR, WD)
        assert same_bits(flats[0].data, want), step
        if n % 2:
            assert same_bits(flats[0].data, p_ag), step
    assert (ties > 0) == (n % 2 == 0)
    st = exs[0].last
    assert st.collectives == 2 * len(ref.buckets)
    assert st.wire_bytes_sent == st.wire_bytes_recv == sum(2 * (n - 1) * t.P for t in exs[0].ts)
    # a tensor crossing a cut is two segments, each chunked from its own start
    assert st.payload_bytes == sum(1024 * t.plan.num_chunks for t in exs[0].ts) \
        >= sum(1024 * b.plan.num_chunks for b in ref.buckets)


# ---- flags --------------------------------------------------------------------------------------
BASE = ["--network", "LeNet", "--dataset", "MNIST", "--compress", "vote", "--optimizer", "lion"]


def test_cli_accepts_the_flag():
    import ewdml

    c = ewdml.parse_args(BASE)
    assert c.vote_exchange == "allgather"
    c = ewdml.parse_args(BASE + ["--vote-exchange", "twostage"])
    assert c.vote_exchange == "twostage" and c.vote_aggregate == "majority"
    assert c.topology == "allgather" and c.error_feedback is False
    c = ewdml.parse_args(BASE + ["--vote-exchange", "twostage", "--hip-graph", "split",
                                 "--clip-grad-norm", "1.0"])
    assert c.hip_graph == "split"
    assert ewdml.parse_args(["--network", "LeNet", "--dataset", "MNIST"]).vote_exchange is None


@pytest.mark.parametrize("flags,reason", [
    (["--vote-exchange", "twostage", "--vote-aggregate", "average"],
     "--vote-exchange twostage .*mean does not fit one bit.*--vote-aggregate average"),
    (["--vote-exchange", "twostage", "--hip-graph", "full"],
     "--vote-exchange twostage .*--hip-graph full"),
    (["--vote-exchange", "twostage", "--hip-graph", "segmented"],
     "--vote-exchange twostage .*--hip-graph segmented"),
    (["--vote-exchange", "twostage", "--topology", "twostage"],
     "--compress vote .*--topology twostage.*--vote-exchange twostage"),
    (["--vote-exchange", "twostage", "--error-feedback"], "--compress vote .*--error-feedback"),
    (["--vote-exchange", "twostage", "--sync-every", "2"], "--compress vote .*--sync-every"),
])
def test_cli_refusals(flags, reason):
    import ewdml

    with pytest.raises(ValueError, match=reason):
        ewdml.parse_args(BASE + flags)


@pytest.mark.parametrize("compress", ["sign", "none", "topk_qsgd"])
def test_cli_flag_belongs_to_the_vote(compress):
    import ewdml

    with pytest.raises(ValueError, match="--vote-exchange belongs to --compress vote"):
        ewdml.parse_args(["--network", "LeNet", "--dataset", "MNIST", "--compress", compress,
                          "--vote-exchange", "twostage"])


def test_hip_graph_auto_resolves_to_split(tmp_path):
    """``--hip-graph auto`` is ``split`` from the flags on; through the trainer on the CPU (no
    graphs there): the exchange and its state in the checkpoint extras."""
    import ewdml
    from ewdml.parallel.twostage import TwoStageVoteExchange
    from ewdml.runtime import Trainer

    cfg = ewdml.parse_args(BASE + ["--vote-exchange", "twostage", "--batch-size", "8",
                                   "--synthetic-size", "64", "--max-steps", "2", "--eval-freq",
                                   "0", "--quiet", "--device", "cpu", "--train-dir",
                                   str(tmp_path)])
    assert cfg.hip_graph == "split"
    assert ewdml.parse_args(BASE).hip_graph == "auto"  # the all-gather vote is not touched
    tr = Trainer(cfg)
    assert isinstance(tr.exchange, TwoStageVoteExchange) and tr.ps_graph
    assert tr.graph_plan is None and tr.flat.attach_grads
    tr.train_step()
    ext = tr.state_extra()
    assert tuple(ext["lion_momentum"].shape) == (1, tr.flat.numel) and "ef_residual" not in ext
    tr.close()


# ---- launches -------------------------------------------------------------------------------------
class _Comm:
    """World of 3 seen from rank 1, collectives stubbed: enough to count launches."""
    world, rank, kind = 3, 1, "stub"

    def __init__(self):
        self.calls = []

    def all_to_all(self, out, inp):
        self.calls.append("all_to_all")
        out.copy_(inp)

    def all_gather(self, out, inp):
        self.calls.append("all_gather")


def _counted(ex):
    calls = []
    for name in ("ts_encode_vote", "ts_vote_reduce", "ts_decode_apply_vote"):
        def wrap(*a, _f=getattr(ex.codec, name), _n=name, **k):
            calls.append((_n, a[0]))
            return _f(*a, **k)
        setattr(ex.codec, name, wrap)
    return calls


def test_three_codec_calls_and_two_collectives_per_bucket_per_step():
    from ewdml.optim.flat import FlatLion
    from ewdml.parallel.twostage import TwoStageVoteExchange

    flat = _flat()
    comm = _Comm()
    ex = TwoStageVoteExchange(flat, comm, make_codec("vote"), FlatLion(flat, lr=LR))
    nb = len(flat.buckets)
    owns = [t.shards[1][2] is not None for t in ex.ts]  # a bucket of < 3 chunks: no shard for rank 1
    assert nb > 1 and sum(owns) >= 2
    calls = _counted(ex)
    for step in range(2):
        del calls[:], comm.calls[:]
        flat.grad.copy_(torch.randn(flat.numel))
        ex.begin()
        ex.finish()
        for b in range(nb):
            assert [n for n, bi in calls if bi == b] == (
                ["ts_encode_vote", "ts_vote_reduce", "ts_decode_apply_vote"] if owns[b] else
                ["ts_encode_vote", "ts_decode_apply_vote"])
        assert len(calls) == 2 * nb + sum(owns)
        assert comm.calls == ["all_to_all", "all_gather"] * nb


def test_an_empty_shard_takes_two_launches_and_sends_a_zero_row():
    from ewdml.optim.flat import FlatLion
    from ewdml.parallel.flat import FlatModel
    from ewdml.parallel.twostage import TwoStageVoteExchange

    flat = FlatModel([torch.nn.Parameter(torch.randn(100))], reverse=False)  # one chunk, 3 ranks
    comm = _Comm()
    ex = TwoStageVoteExchange(flat, comm, make_codec("vote"), FlatLion(flat, lr=LR))
    assert ex.ts[0].shards[1][2] is None and ex.ts[0].shards[2][2] is not None
    calls = _counted(ex)
    flat.grad.copy_(-torch.rand(flat.numel) - 1)  # every element votes -1
    ex.begin()
    ex.finish()
    assert [n for n, _ in calls] == ["ts_encode_vote", "ts_decode_apply_vote"]
    assert comm.calls == ["all_to_all", "all_gather"]
    assert int(ex.own[0].max()) == 0  # the row this rank contributes to the all-gather
    assert int(ex.send[0][2].max()) > 0 and int(ex.send[0][:2].max()) == 0


def test_the_exchange_refuses_what_it_cannot_carry():
    from ewdml.optim.flat import FlatLion, FlatSGD
    from ewdml.parallel.twostage import TwoStageVoteExchange

    flat = _flat()
    with pytest.raises(ValueError, match="mean does not fit"):
        TwoStageVoteExchange(flat, _Comm(), make_codec("vote", aggregate="average"),
                             FlatLion(flat))
    with pytest.raises(ValueError, match="vote codec"):
        TwoStageVoteExchange(flat, _Comm(), make_codec("sign"), FlatLion(flat))
    with pytest.raises(ValueError, match="only Lion"):
        TwoStageVoteExchange(flat, _Comm(), make_codec("vote"), FlatSGD(flat, lr=0.1))
    with pytest.raises(ValueError, match="kind 'sign'"):
        make_codec("sign").bind_twostage(
            [TwoStagePlan(b.plan, shard_plans(b.plan, 2, b.start), kind="vote")
             for b in flat.buckets], "cpu")
