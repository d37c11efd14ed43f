"""The two-stage vote's HIP kernels (ops/csrc/lion.hip: the slot-addressed k_lion_encode and
k_lion_vote_apply, and k_vote_reduce) vs the torch oracle, on one MI355X.

Exactness contract: row bytes, momenta, parameters and the bf16 shadow are bitwise the oracle's
(``oracle.encode_vote`` / ``vote_reduce`` / ``vote_apply`` per shard): the floating-point part is
the all-gather vote's, rounded operation by operation on both sides, and the owner step is integer.

One bucket of tensors with word and chunk tails (3, 70, 8191, 8193, 2 * 8192 + 5) and one whose
gradient is identically zero, cut for 1, 2, 3, 4 and 11 ranks (11: more ranks than chunks, so some
shards are empty).  The row buffers are filled with a sentinel: every byte outside the slots must
survive.  Both sides run through the codec (``Codec.ts_*``), bound to the CPU and to the GPU."""
import pytest
import torch

from ewdml import ops
from ewdml.compress import make_codec, oracle
from ewdml.compress.plan import BucketPlan, TwoStagePlan
from ewdml.compress.rng import stream_key
from ewdml.parallel.sharded import shard_plans

pytestmark = pytest.mark.gpu

DEV = "cuda"
NUMELS = [2 * 8192 + 5, 3, 8191, 8193, 70, 100]
ZERO_TENSOR = 5
WORLDS = [1, 2, 3, 4, 11]
SENTINEL = -12345.0
FILL = 0xA5
BETAS = (0.9, 0.99)


def _plan():
    offs, o = [], 0
    for n in NUMELS:
        offs.append(o)
        o += (n + 63) // 64 * 64
    return BucketPlan(NUMELS, offs, 1.0, 4096, o)


PLAN = _plan()
INSIDE = torch.zeros(PLAN.length, dtype=torch.bool)
for _o, _n in zip(PLAN.offsets, PLAN.numels):
    INSIDE[_o:_o + _n] = True
_TS, _CODECS = {}, {}


def _ts(n):
    if n not in _TS:
        _TS[n] = TwoStagePlan(PLAN, shard_plans(PLAN, n, PLAN.bucket_offset), kind="vote")
    return _TS[n]


def _codec(n, device):
    if (n, device) not in _CODECS:
        _CODECS[(n, device)] = make_codec("vote", seed=5).bind_twostage([_ts(n)], device)
    return _CODECS[(n, device)]


def _used(ts):
    """bool [N * P]: the bytes the slot table addresses."""
    used = torch.zeros(ts.N * ts.P, dtype=torch.bool)
    for _, w in ts.slots:
        used[w:w + 1024] = True
    return used


def _same(a, b):
    return torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def _rand(seed, scale=1.0, bf16=False):
    """Random values inside the tensors (exact zeros planted at even and odd indices, the last
    tensor all zero), the sentinel between them."""
    g = torch.full((PLAN.length,), SENTINEL)
    gen = torch.Generator().manual_seed(seed)
    for t, (off, n) in enumerate(zip(PLAN.offsets, PLAN.numels)):
        v = torch.randn(n, generator=gen) * scale
        if bf16:
            v = v.to(torch.bfloat16).float()
        for i in (0, 1, 30, 31, 32, 8190, 8191, 8192, 8193, n - 2, n - 1):
            if 0 <= i < n:
                v[i] = 0.0
        g[off:off + n] = 0.0 if t == ZERO_TENSOR else v
    return g


def _zero_like_planted(m, g):
    """The momentum is zero where the gradient is: c = 0 there and the dither decides."""
    return torch.where(g == 0, torch.zeros_like(m), m)


def test_the_cuts_cover_the_cases():
    assert _ts(1).plan.num_chunks < _ts(4).plan.num_chunks  # cuts add segments
    assert all(sp is not None for _, _, sp, _, _ in _ts(4).shards)
    empty = [sp is None for _, _, sp, _, _ in _ts(11).shards]
    assert any(empty) and not all(empty)


# ---- push -------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["flat", "bf16_pointers"])
@pytest.mark.parametrize("n", WORLDS)
def test_encode_matches_oracle(n, mode):
    ops.require()
    ts, rank, step = _ts(n), n - 1, 3
    g = _rand(20, 0.3, bf16=mode != "flat")
    m = _zero_like_planted(_rand(21, 2.0), g)
    rows_ref = torch.full((n, ts.P), FILL, dtype=torch.uint8)
    m_ref = m.clone()
    _codec(n, "cpu").ts_encode_vote(0, g, rows_ref, m_ref, BETAS, step, rank)
    used = _used(ts)
    assert bool((rows_ref.view(-1)[~used] == FILL).all())

    rows = torch.full((n, ts.P), FILL, dtype=torch.uint8, device=DEV)
    m_dev = m.to(DEV)
    if mode == "flat":
        grad = g.to(DEV)
    else:  # one bf16 tensor per segment of the shard-major plan, read in place
        grad = [g[o:o + k].to(torch.bfloat16).to(DEV)
                for o, k in zip(ts.plan.offsets, ts.plan.numels)]
    st = torch.tensor([step - 1], dtype=torch.int32, device=DEV)  # the device counter decides
    _codec(n, DEV).ts_encode_vote(0, grad, rows, m_dev, BETAS, 12345, rank, step_tensor=st)
    got = rows.cpu()
    assert bool((got.view(-1)[~used] == FILL).all()), "bytes outside the slots were written"
    assert torch.equal(got, rows_ref), \
        f"rows differ at bytes {(got != rows_ref).view(-1).nonzero()[:10].flatten().tolist()}"
    got_m = m_dev.cpu()
    assert _same(got_m, m_ref) and bool((got_m[~INSIDE] == SENTINEL).all())
    assert not _same(got_m[INSIDE], m[INSIDE]) and int(st) == step - 1
    for r, (_, _, sp, _, _) in enumerate(ts.shards):  # an empty shard's row is never written
        if sp is None:
            assert bool((got[r] == FILL).all())


def test_encode_in_a_graph_follows_the_device_step():
    """Captured once, replayed twice: the second replay votes with step 2, so the identically
    zero tensor's bits flip (dither parity) and the momentum has moved twice."""
    ops.require()
    n, rank = 3, 1
    ts = _ts(n)
    g = _rand(30, 0.3)
    m = _zero_like_planted(_rand(31, 2.0), g)
    m_ref, refs = m.clone(), []
    for step in (1, 2):
        rows_ref = torch.zeros((n, ts.P), dtype=torch.uint8)
        _codec(n, "cpu").ts_encode_vote(0, g, rows_ref, m_ref, BETAS, step, rank)
        refs.append(rows_ref)
    assert not torch.equal(refs[0], refs[1])

    rows = torch.zeros((n, ts.P), dtype=torch.uint8, device=DEV)
    grad, m_dev = g.to(DEV), m.to(DEV)
    st = torch.zeros(1, dtype=torch.int32, device=DEV)
    codec = _codec(n, DEV)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        codec.ts_encode_vote(0, grad, rows, m_dev, BETAS, 12345, rank, step_tensor=st)
    assert _same(m_dev.cpu(), m)  # a capture runs nothing
    for i in range(2):
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(rows.cpu(), refs[i]), f"replay {i}"
        st.add_(1)
    assert _same(m_dev.cpu(), m_ref)


# ---- owner step ---------------------------------------------------------------------------------
def _votes(n, ts, seed):
    """[N, P] rows of random words with ties (even N), all-set and all-clear words in every
    shard's range; the bytes past a shard's payload keep the fill."""
    gen = torch.Generator().manual_seed(seed)
    recv = torch.full((n, ts.P), FILL, dtype=torch.uint8)
    words = torch.randint(0, 256, (n, ts.P), generator=gen, dtype=torch.int64).to(torch.uint8)
    if n % 2 == 0:  # the second half of the rows votes against the first
        words[n // 2:, :512] = ~words[:n // 2, :512]
    words[:, 512:640] = 0xFF
    words[:, 640:768] = 0
    return recv, words


@pytest.mark.parametrize("n", WORLDS)
def test_vote_reduce_matches_oracle(n):
    ops.require()
    ts = _ts(n)
    cpu, dev = _codec(n, "cpu"), _codec(n, DEV)
    ties = 0
    for r, (_, _, sp, lay, _) in enumerate(ts.shards):
        if sp is None:
            with pytest.raises(ValueError, match="empty shard"):
                dev.ts_vote_reduce(0, r, torch.zeros((n, ts.P), dtype=torch.uint8, device=DEV),
                                   torch.zeros(ts.P, dtype=torch.uint8, device=DEV))
            continue
        recv, words = _votes(n, ts, 40 + r)
        recv[:, :lay.nbytes] = words[:, :lay.nbytes]
        out_ref = torch.full((ts.P,), FILL, dtype=torch.uint8)
        cpu.ts_vote_reduce(0, r, recv, out_ref)
        s = oracle.vote_counts(recv, sp, lay)
        ties += int((s == 0).sum())
        rd = recv.to(DEV)
        out = torch.full((ts.P,), FILL, dtype=torch.uint8, device=DEV)
        dev.ts_vote_reduce(0, r, rd, out)
        got = out.cpu()
        assert torch.equal(got, out_ref), \
            f"shard {r}: bytes {(got != out_ref).nonzero()[:10].flatten().tolist()}"
        assert bool((got[lay.nbytes:] == FILL).all())  # nothing past the shard's words
        assert torch.equal(rd.cpu(), recv)  # only read
        assert bool((got[512:640] == 0xFF).all()) and bool((got[640:768] == 0).all())
        if n % 2 == 0:  # a tie takes the owner's own vote
            assert torch.equal(got[:512], recv[r, :512])
    assert (ties > 0) == (n % 2 == 0)


# ---- pull ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("shadow", [False, True])
@pytest.mark.parametrize("wd", [0.0, 0.1])
@pytest.mark.parametrize("n", WORLDS)
def test_apply_matches_oracle(n, wd, shadow):
    ops.require()
    ts = _ts(n)
    gen = torch.Generator().manual_seed(60 + n)
    rows = torch.randint(0, 256, (n, ts.P), generator=gen, dtype=torch.int64).to(torch.uint8)
    p0 = _rand(9)
    lrs = (1e-3, 3e-4)  # the device lr changes between the two calls
    p = p0.clone()
    for lr in lrs:
        _codec(n, "cpu").ts_decode_apply_vote(0, rows, p, dict(lr=lr, weight_decay=wd))
    pd, rd = p0.to(DEV), rows.to(DEV)
    sh = torch.full((PLAN.length,), 7.0, dtype=torch.bfloat16, device=DEV) if shadow else None
    lr_t = torch.tensor([lrs[0]], dtype=torch.float32, device=DEV)
    step, rank = 41, 3
    ks = torch.tensor([step, 0], dtype=torch.int32, device=DEV)
    hp = dict(lr=77.0, weight_decay=wd, lr_t=lr_t)
    dev = _codec(n, DEV)
    dev.ts_decode_apply_vote(0, rd, pd, hp, shadow=sh, key_state=ks, rank=rank)
    lr_t.fill_(lrs[1])
    dev.ts_decode_apply_vote(0, rd, pd, hp, shadow=sh, rank=rank)
    got = pd.cpu()
    assert _same(got, p)
    assert bool((got[~INSIDE] == SENTINEL).all()) and not _same(got[INSIDE], p0[INSIDE])
    if wd == 0.0:  # every element moved by exactly +-lr, twice: no zero direction
        assert bool(((got - p0)[INSIDE] != 0).all())
    if shadow:
        shc = sh.cpu()
        assert torch.equal(shc[INSIDE], got[INSIDE].to(torch.bfloat16))
        assert bool((shc[~INSIDE] == 7.0).all())
    assert torch.equal(rd.cpu(), rows)  # only read
    assert [int(x) & 0xFFFFFFFF for x in ks.cpu()] == [step + 1, stream_key(5, step + 1, rank)]


def test_wrappers_refuse_buffers_that_do_not_hold_the_slots():
    ops.require()
    n = 3
    ts, dev = _ts(n), _codec(n, DEV)
    sl = dev.ts_dev[0]
    small = torch.zeros(n * ts.P - 16, dtype=torch.uint8, device=DEV)
    m = torch.zeros(PLAN.length, device=DEV)
    with pytest.raises(ValueError, match="slot table addresses"):
        ops.lion_encode(sl, m, small, None, m, 0.9, 0.99, 1, 0, slots=sl)
    with pytest.raises(ValueError, match="slot table addresses"):
        ops.lion_vote_apply(sl, small, None, m, 1e-3, slots=sl)
    with pytest.raises(ValueError, match="majority"):
        ops.lion_vote_apply(sl, torch.zeros(n * ts.P, dtype=torch.uint8, device=DEV), None, m,
                            1e-3, aggregate="average", slots=sl)
    sign = ops.SignSlots(TwoStagePlan(PLAN, shard_plans(PLAN, n, PLAN.bucket_offset)), DEV)
    with pytest.raises(ValueError, match="vote two-stage plan"):
        ops.lion_encode(sign, m, torch.zeros(sign.nbytes, dtype=torch.uint8, device=DEV), None,
                        m, 0.9, 0.99, 1, 0, slots=sign)
    _, _, sp, lay, _ = ts.shards[0]
    tab = dev.ts_shard_dev[0][0]
    recv = torch.zeros((n, ts.P), dtype=torch.uint8, device=DEV)
    with pytest.raises(ValueError, match="out too small"):
        ops.vote_reduce(tab, recv, lay, 0, torch.zeros(lay.nbytes - 16, dtype=torch.uint8,
                                                       device=DEV))
    with pytest.raises(ValueError, match="owner row"):
        ops.vote_reduce(tab, recv, lay, n, torch.zeros(ts.P, dtype=torch.uint8, device=DEV))
    with pytest.raises(ValueError, match="row stride"):
        ops.vote_reduce(tab, recv[:, :lay.nbytes - 16].contiguous(), lay, 0,
                        torch.zeros(ts.P, dtype=torch.uint8, device=DEV))
