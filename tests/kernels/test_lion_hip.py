"""Lion's HIP kernels (ops/csrc/lion.hip: k_lion_flat, k_lion_encode, k_lion_vote_apply) vs the
torch oracle, on one MI355X.

Exactness contract: payload bytes, momenta, parameters and the bf16 shadow are bitwise the
oracle's (``oracle.lion_apply`` / ``encode_vote`` / ``vote_apply``): every operation is rounded
separately on both sides, the vote is counted in integers, and the file set is built with
-ffp-contract=off.

Every test uses one bucket whose tensors sit on word boundaries (1, 31, 33), on chunk boundaries
with their tails (8191, 8192, 8193) and over several chunks (2 * 8192 + 5); the space between the
tensors holds a sentinel that must survive."""
import pytest
import torch

from ewdml import ops
from ewdml.compress import oracle
from ewdml.compress.plan import BucketPlan, Layout
from ewdml.compress.rng import stream_key

pytestmark = pytest.mark.gpu

DEV = "cuda"
NUMELS = [1, 31, 33, 8191, 8192, 8193, 2 * 8192 + 5]
SENTINEL = -12345.0
B1, B2 = 0.9, 0.99


def _plan():
    offs, o = [], 0
    for n in NUMELS:
        offs.append(o)
        o += (n + 63) // 64 * 64
    return BucketPlan(NUMELS, offs, 1.0, 4096, o)


PLAN = _plan()
LAY = Layout.build("vote", PLAN)
INSIDE = torch.zeros(PLAN.length, dtype=torch.bool)
for _o, _n in zip(PLAN.offsets, PLAN.numels):
    INSIDE[_o:_o + _n] = True


def _rand(seed, scale=1.0):
    """Random values without exact zeros inside the tensors, the sentinel between them."""
    g = torch.full((PLAN.length,), SENTINEL)
    gen = torch.Generator().manual_seed(seed)
    for off, n in zip(PLAN.offsets, PLAN.numels):
        v = torch.randn(n, generator=gen) * scale
        g[off:off + n] = torch.where(v == 0, torch.full_like(v, 0.5), v)
    return g


def _same(a, b):
    return torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def _planted(seed):
    """Gradient and momentum with exact zeros in both at even and odd indices of every tensor
    (first, last and chunk-crossing elements), -0.0 and one NaN."""
    g, m = _rand(seed, 0.3), _rand(seed + 1, 2.0)
    for off, n in zip(PLAN.offsets, PLAN.numels):
        for i in (0, 1, 6, 7, 30, 31, 32, 8190, 8191, 8192, 8193, n - 2, n - 1):
            if 0 <= i < n:
                g[off + i] = 0.0
                m[off + i] = 0.0
        if n > 40:
            g[off + 12], m[off + 12] = -0.0, -0.0
            g[off + 13], m[off + 13] = -0.0, 0.0
            g[off + 21], m[off + 21] = 0.0, -3.0
    g[PLAN.offsets[-1] + 8192 + 77] = float("nan")
    return g, m


# the oracle runs once per case on the CPU and is shared by the pointer-mode and flat-view tests
_ENC = {}


def _encode_ref(step, rank):
    if (step, rank) not in _ENC:
        g, m = _planted(20)
        m_ref = m.clone()
        pay = oracle.encode_vote(g, PLAN, LAY, m_ref, B1, B2, step, rank)
        _ENC[(step, rank)] = (g, m, pay, m_ref)
    return _ENC[(step, rank)]


@pytest.mark.parametrize("mode", ["flat", "pointers"])
@pytest.mark.parametrize("rank", [0, 1])
@pytest.mark.parametrize("step", [1, 2])
def test_encode_matches_oracle(step, rank, mode):
    ops.require()
    g, m, pay_ref, m_ref = _encode_ref(step, rank)
    dp = ops.DevicePlan(PLAN, DEV)
    pay = torch.full((LAY.nbytes,), 0xFF, dtype=torch.uint8, device=DEV)  # every word is rewritten
    m_dev = m.to(DEV)
    if mode == "flat":
        grad = g.to(DEV)
    else:
        grad = [g[o:o + n].clone().to(DEV) for o, n in zip(PLAN.offsets, PLAN.numels)]
    # the host step and the device counter (step - 1 before the step) give the same payload
    if rank == 0:
        ops.lion_encode(dp, grad, pay, LAY, m_dev, B1, B2, step, rank)
    else:
        st = torch.tensor([step - 1], dtype=torch.int32, device=DEV)
        ops.lion_encode(dp, grad, pay, LAY, m_dev, B1, B2, 12345, rank, step_tensor=st)
        assert int(st) == step - 1
    got = pay.cpu()
    assert got.numel() == 1024 * PLAN.num_chunks
    assert torch.equal(got, pay_ref), \
        f"payload differs at bytes {(got != pay_ref).nonzero()[:10].flatten().tolist()}"
    got_m = m_dev.cpu()
    ok = INSIDE & ~torch.isnan(m_ref)
    assert _same(got_m[ok], m_ref[ok]) and bool(torch.isnan(got_m[INSIDE & ~ok]).all())
    assert bool((got_m[~INSIDE] == SENTINEL).all())
    if mode == "flat":
        assert _same(grad.cpu()[~torch.isnan(g)], g[~torch.isnan(g)])  # only read


def test_encode_bf16_pointers():
    ops.require()
    g, m = _rand(3, 0.3), _rand(4)
    for o, n in zip(PLAN.offsets, PLAN.numels):
        g[o:o + n] = g[o:o + n].to(torch.bfloat16).float()
    grads = [g[o:o + n].clone().to(torch.bfloat16).to(DEV)
             for o, n in zip(PLAN.offsets, PLAN.numels)]
    m_ref = m.clone()
    ref = oracle.encode_vote(g, PLAN, LAY, m_ref, B1, B2, 5, 0)
    dp = ops.DevicePlan(PLAN, DEV)
    pay = torch.zeros(LAY.nbytes, dtype=torch.uint8, device=DEV)
    m_dev = m.to(DEV)
    ops.lion_encode(dp, grads, pay, LAY, m_dev, B1, B2, 5, 0)
    assert torch.equal(pay.cpu(), ref) and _same(m_dev.cpu(), m_ref)


_ROWS = {}


def _rows(N):
    """N random vote payloads (beta = 0: the sign of a random gradient; zeros dithered)."""
    if N not in _ROWS:
        rows = []
        for r in range(N):
            g = _rand(100 + r)
            g[::11] = 0.0
            rows.append(oracle.encode_vote(g, PLAN, LAY, torch.zeros(PLAN.length), 0.0, 0.0, 1, r))
        _ROWS[N] = torch.stack(rows)
    return _ROWS[N]


@pytest.mark.parametrize("wd", [0.0, 0.1])
@pytest.mark.parametrize("aggregate", ["majority", "average"])
@pytest.mark.parametrize("N", [1, 2, 3, 8])
def test_vote_apply_matches_oracle(N, aggregate, wd):
    ops.require()
    recv = _rows(N)
    p0 = _rand(9)
    lrs = (1e-3, 3e-4)  # the device lr changes between the two calls
    p = p0.clone()
    for lr in lrs:
        oracle.vote_apply(recv, PLAN, LAY, p, lr, wd, aggregate, 1.0 / N)
    dp = ops.DevicePlan(PLAN, DEV)
    pd, rd = p0.to(DEV), recv.to(DEV)
    sh = torch.full((PLAN.length,), 7.0, dtype=torch.bfloat16, device=DEV)
    lr_t = torch.tensor([lrs[0]], dtype=torch.float32, device=DEV)
    seed, step, rank = 5, 41, 3
    ks = torch.tensor([step, 0], dtype=torch.int32, device=DEV)
    ops.lion_vote_apply(dp, rd, LAY, pd, 77.0, wd, aggregate, shadow=sh, lr_tensor=lr_t,
                        key_state=ks, key_seed=seed, key_rank=rank)
    lr_t.fill_(lrs[1])
    ops.lion_vote_apply(dp, rd, LAY, pd, 77.0, wd, aggregate, shadow=sh, lr_tensor=lr_t)
    got = pd.cpu()
    ulp = (got.view(torch.int32) - p.view(torch.int32)).abs().max()
    print(f"N={N} {aggregate} wd={wd}: max param difference {int(ulp)} ulp")
    assert _same(got, p)
    assert bool((got[~INSIDE] == SENTINEL).all()) and not _same(got[INSIDE], p0[INSIDE])
    shc = sh.cpu()
    assert torch.equal(shc[INSIDE], got[INSIDE].to(torch.bfloat16))
    assert bool((shc[~INSIDE] == 7.0).all())
    assert torch.equal(rd.cpu(), recv)  # only read
    assert [int(x) & 0xFFFFFFFF for x in ks.cpu()] == [step + 1, stream_key(seed, step + 1, rank)]
    if N == 2:  # ties exist and leave p where weight decay alone puts it
        tie = (oracle.vote_counts(recv, PLAN, LAY) == 0).any()
        assert bool(tie)


def test_vote_apply_host_lr():
    ops.require()
    recv, p0 = _rows(3), _rand(9)
    p = p0.clone()
    oracle.vote_apply(recv, PLAN, LAY, p, 2e-3, 0.1, "majority", 1.0 / 3)
    pd = p0.to(DEV)
    ops.lion_vote_apply(ops.DevicePlan(PLAN, DEV), recv.to(DEV), LAY, pd, 2e-3, 0.1)
    assert _same(pd.cpu(), p)


@pytest.mark.parametrize("wd", [0.0, 0.1])
@pytest.mark.parametrize("grad_scale", [1.0, 1.0 / 3.0])
def test_lion_flat_matches_oracle_whole_and_per_bucket(grad_scale, wd):
    """The dense step over the whole range (odd length: scalar tail), and the same range cut into
    'buckets' at 16-byte boundaries with odd tails: bitwise the oracle both ways."""
    ops.require()
    n = PLAN.length + 3
    gen = torch.Generator().manual_seed(31)
    p0, m0, g = (torch.randn(n, generator=gen) for _ in range(3))
    g[5], m0[5] = 0.0, 0.0  # c == 0: no sign step
    g[6] = float("nan")
    lr = 1e-3
    p, m = p0.clone(), m0.clone()
    gs = g * torch.tensor(grad_scale, dtype=torch.float32)
    for _ in range(2):
        oracle.lion_apply(p, m, gs, lr, B1, B2, wd)
    lr_t = torch.tensor([lr], dtype=torch.float32, device=DEV)
    # whole range
    pw, mw, gd = p0.to(DEV), m0.to(DEV), g.to(DEV)
    sh = torch.zeros(n, dtype=torch.bfloat16, device=DEV)
    for _ in range(2):
        ops.lion_flat(pw, mw, gd, 77.0, B1, B2, wd, grad_scale, shadow=sh, lr_tensor=lr_t)
    fin = ~torch.isnan(m)  # the NaN gradient poisons its momentum and takes no sign step
    assert _same(pw.cpu(), p) and _same(mw.cpu()[fin], m[fin])
    assert bool(torch.isnan(mw.cpu()[~fin]).all()) and int((~fin).sum()) == 1
    assert torch.equal(sh.cpu(), pw.cpu().to(torch.bfloat16))
    # per bucket: cuts at multiples of 4 elements, the last range ends on the odd tail
    cuts = [0, 4, 8192 + 64, 3 * 8192, n]
    pb, mb = p0.to(DEV), m0.to(DEV)
    for _ in range(2):
        for a, b in zip(cuts, cuts[1:]):
            ops.lion_flat(pb[a:b], mb[a:b], gd[a:b], lr, B1, B2, wd, grad_scale)
    assert _same(pb.cpu(), pw.cpu()) and _same(mb.cpu()[fin], mw.cpu()[fin])


def test_lion_flat_bf16_gradient():
    ops.require()
    n = 8192 + 6
    gen = torch.Generator().manual_seed(32)
    p0, m0 = torch.randn(n, generator=gen), torch.randn(n, generator=gen)
    g = torch.randn(n, generator=gen).to(torch.bfloat16)
    p, m = p0.clone(), m0.clone()
    oracle.lion_apply(p, m, g.float() * torch.tensor(0.5), 1e-3, B1, B2, 0.1)
    pd, md = p0.to(DEV), m0.to(DEV)
    ops.lion_flat(pd, md, g.to(DEV), 1e-3, B1, B2, 0.1, 0.5)
    assert _same(pd.cpu(), p) and _same(md.cpu(), m)


@pytest.mark.parametrize("wd", [0.0, 0.1])
def test_encode_then_apply_at_one_rank_is_lion_flat(wd):
    """N = 1 on inputs with no exact zero c: the vote path and k_lion_flat agree bit for bit, and
    a captured encode + apply + counter increment replays to the same state."""
    ops.require()
    dp = ops.DevicePlan(PLAN, DEV)
    p0, m0 = _rand(1), _rand(2)
    grads = [_rand(10 + i, 0.3) for i in range(3)]
    lr = 1e-3
    lr_t = torch.tensor([lr], dtype=torch.float32, device=DEV)
    # dense: per tensor, so the sentinels between the tensors are not stepped
    pf, mf = p0.to(DEV), m0.to(DEV)
    for g in grads:
        gd = g.to(DEV)
        for o, n in zip(PLAN.offsets, PLAN.numels):
            ops.lion_flat(pf[o:o + n], mf[o:o + n], gd[o:o + n], lr, B1, B2, wd)

    def state():
        return dict(g=torch.zeros(PLAN.length, device=DEV), p=p0.to(DEV), m=m0.to(DEV),
                    t=torch.zeros(1, dtype=torch.int32, device=DEV),
                    pay=torch.zeros(1, LAY.nbytes, dtype=torch.uint8, device=DEV))

    def step(s):
        ops.lion_encode(dp, s["g"], s["pay"][0], LAY, s["m"], B1, B2, 0, 0, step_tensor=s["t"])
        ops.lion_vote_apply(dp, s["pay"], LAY, s["p"], 0.0, wd, "majority", lr_tensor=lr_t)
        s["t"].add_(1)

    eager = state()
    for g in grads:
        eager["g"].copy_(g)
        step(eager)
    assert _same(eager["p"].cpu(), pf.cpu()) and _same(eager["m"].cpu(), mf.cpu())
    assert bool((eager["p"].cpu()[~INSIDE] == SENTINEL).all())
    cap = state()
    cap["g"].copy_(grads[0])
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        with torch.cuda.graph(graph, stream=side):
            step(cap)
    torch.cuda.current_stream().wait_stream(side)
    graph.replay()  # capturing does not run: this is the first step
    for g in grads[1:]:
        cap["g"].copy_(g)
        graph.replay()
    torch.cuda.synchronize()
    assert int(cap["t"]) == 3
    for k in ("p", "m", "pay"):
        assert torch.equal(cap[k], eager[k]), k


def test_zero_gradient_dither_follows_the_device_step():
    """An identically zero gradient and momentum: the votes alternate with the device counter, so
    two replayed steps cancel."""
    ops.require()
    dp = ops.DevicePlan(PLAN, DEV)
    g = torch.zeros(PLAN.length, device=DEV)
    m = torch.zeros(PLAN.length, device=DEV)
    p0 = torch.round(_rand(1) * 8) / 8  # multiples of 1/8: p -/+ 1/4 is exact
    p = p0.to(DEV)
    t = torch.zeros(1, dtype=torch.int32, device=DEV)
    pay = torch.zeros(1, LAY.nbytes, dtype=torch.uint8, device=DEV)
    seen = []
    for _ in range(2):
        ops.lion_encode(dp, g, pay[0], LAY, m, B1, B2, 0, 0, step_tensor=t)
        ops.lion_vote_apply(dp, pay, LAY, p, 0.25)
        t.add_(1)
        seen.append(pay.clone())
    assert not torch.equal(seen[0], seen[1])
    assert torch.equal(p.cpu(), p0) and not m.any()  # by value: -0.0 + 1/4 - 1/4 is +0.0


def test_bad_operands_rejected():
    """Size, dtype, alignment and layout kind are checked on the host, before any launch."""
    ops.require()
    dp = ops.DevicePlan(PLAN, DEV)
    g, m, p = (torch.zeros(PLAN.length, device=DEV) for _ in range(3))
    pay = torch.zeros(LAY.nbytes, dtype=torch.uint8, device=DEV)
    big = torch.zeros(PLAN.length + 4, device=DEV)
    bigpay = torch.zeros(LAY.nbytes + 16, dtype=torch.uint8, device=DEV)
    sign = Layout.build("sign", PLAN)
    enc, dec = ops.lion_encode, ops.lion_vote_apply
    with pytest.raises(ValueError):  # another codec's layout
        enc(dp, g, pay, sign, m, B1, B2, 1, 0)
    with pytest.raises(ValueError):  # too short
        enc(dp, g, pay[:LAY.nbytes - 16], LAY, m, B1, B2, 1, 0)
    with pytest.raises(ValueError):
        enc(dp, g, pay, LAY, m[:100], B1, B2, 1, 0)
    with pytest.raises(ValueError):
        enc(dp, g[:100], pay, LAY, m, B1, B2, 1, 0)
    with pytest.raises(TypeError):  # wrong dtypes
        enc(dp, g, pay, LAY, m.double(), B1, B2, 1, 0)
    with pytest.raises(TypeError):
        enc(dp, g, pay, LAY, m, B1, B2, 1, 0, step_tensor=torch.zeros(1, device=DEV))
    with pytest.raises(ValueError):  # misaligned views
        enc(dp, g, pay, LAY, big[1:], B1, B2, 1, 0)
    with pytest.raises(ValueError):
        enc(dp, g, bigpay[4:], LAY, m, B1, B2, 1, 0)
    recv = pay[None]
    with pytest.raises(ValueError):  # row length is not the layout's
        dec(dp, bigpay[None], LAY, p, 1e-3)
    with pytest.raises(ValueError):
        dec(dp, recv, sign, p, 1e-3)
    with pytest.raises(ValueError):
        dec(dp, recv, LAY, p[:100], 1e-3)
    with pytest.raises(ValueError):
        dec(dp, recv, LAY, p, 1e-3, aggregate="median")
    with pytest.raises(TypeError):
        dec(dp, recv, LAY, p.double(), 1e-3)
    with pytest.raises(TypeError):
        dec(dp, recv, LAY, p, 1e-3, shadow=torch.zeros(PLAN.length, device=DEV))
    with pytest.raises(ValueError):
        dec(dp, recv, LAY, big[1:], 1e-3)
    with pytest.raises(ValueError):  # dense step: sizes, alignment, dtype
        ops.lion_flat(p, m[:100], g, 1e-3, B1, B2)
    with pytest.raises(ValueError):
        ops.lion_flat(big[1:], big[1:], big[1:], 1e-3, B1, B2)
    with pytest.raises(TypeError):
        ops.lion_flat(p, m, g.double(), 1e-3, B1, B2)
    torch.cuda.synchronize()
    for t in (pay, g, m, p):
        assert not t.any()  # nothing ran
