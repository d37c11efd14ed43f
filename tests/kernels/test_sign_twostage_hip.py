"""The two-stage sign all-reduce's three launches (ops/csrc/sign_codec.hip: the slot-addressed
k_sign_encode, k_sign_reduce_encode, and the slot-addressed k_sign_decode_apply /
k_sign_decode_onebit) vs the torch oracle, on one MI355X.

Exactness contract: row-buffer bytes (pads included: they stay 0), both residuals, parameters,
momentum / ``exp_avg`` and the bf16 shadow are bitwise the oracle's.  The reference of every test
is the same ``Codec`` bound on the CPU, where it dispatches to ``compress/oracle.py``.

Tensor sizes {1, 31, 8192, 8193, 20000}: a lone element, a sub-float4 tail, an exact chunk, a chunk
plus one, three chunks with a partial last.  Cut into 2 shards the cut falls inside the 8193
tensor, into 3 shards inside the 8192 and the 20000 tensors.  The SGD step uses lr = 2^-4 and
dampening 0, so the torch reference does not depend on fma contraction.
"""
import pytest
import torch

from ewdml import ops
from ewdml.compress import BucketPlan, TwoStagePlan, make_codec, oracle
from ewdml.parallel.sharded import shard_plans

pytestmark = pytest.mark.gpu

DEV = "cuda"
SIZES = [1, 31, 8192, 8193, 20000]
HP = dict(lr=2.0 ** -4, momentum=0.5, dampening=0.0, weight_decay=2.0 ** -7, nesterov=False)


def _plan(numels=SIZES, start=4096):
    offs, o = [], 0
    for n in numels:
        offs.append(o)
        o += (n + 63) // 64 * 64
    return BucketPlan(numels, offs, 1.0, start, o)


def _pair(shards):
    """(TwoStagePlan, CPU codec = the oracle, GPU codec = the kernels)."""
    plan = _plan()
    ts = TwoStagePlan(plan, shard_plans(plan, shards, plan.bucket_offset))
    return (ts, make_codec("sign").bind_twostage([ts], "cpu"),
            make_codec("sign").bind_twostage([ts], DEV))


def _vec(plan, seed, scale=1.0):
    g = torch.zeros(plan.length)
    gen = torch.Generator().manual_seed(seed)
    for off, n in zip(plan.offsets, plan.numels):
        g[off:off + n] = torch.randn(n, generator=gen) * (0.1 + torch.rand(1, generator=gen))
    return g * scale


def _bits(a, b):
    return a.shape == b.shape and torch.equal(a.cpu().contiguous().view(torch.int32),
                                              b.cpu().contiguous().view(torch.int32))


def _rows(ts, fill=0):
    return torch.full((ts.N, ts.P), fill, dtype=torch.uint8)


@pytest.fixture(scope="module")
def pushed():
    """Per shard count: rows produced by the oracle push of one gradient (shared, read only)."""
    out = {}
    for s in (1, 2, 3):
        ts, cpu, _ = _pair(s)
        rows = _rows(ts)
        cpu.ts_encode(0, _vec(ts.plan, 11), rows, torch.zeros(ts.plan.length))
        out[s] = rows
    return out


@pytest.mark.parametrize("mom", [None, 0.0, 2.0 ** -5])  # plain | momentum push, wd off | on
@pytest.mark.parametrize("shards", [1, 2, 3])
def test_push_encode_matches_oracle(shards, mom):
    ops.require()
    ts, cpu, gpu = _pair(shards)
    plan = ts.plan
    if shards == 3:  # uneven shards: the rows are wider than the smallest payload
        assert ts.P > min(lay.nbytes for _, _, _, lay, _ in ts.shards)
    r_ref = _vec(plan, 50, 0.3)
    m, p = _vec(plan, 70, 2.0), _vec(plan, 71, 30.0)
    r_dev, m_dev, p_dev = r_ref.to(DEV), m.to(DEV), p.to(DEV)
    rows_ref, rows_dev = _rows(ts), _rows(ts).to(DEV)
    for it in range(2):
        g = _vec(plan, 5 + it)
        if it == 0:
            s, n = plan.chunk_start[2], plan.chunk_len[2]  # an all-zero chunk: scale 0
            g[s:s + n] = 0.0
            r_ref[s:s + n] = 0.0
            m[s:s + n] = 0.0
            p[s:s + n] = 0.0
            s = plan.chunk_start[3]  # -0.0 inputs: e = -0.0, bit 0
            g[s:s + 8] = -0.0
            r_ref[s:s + 8] = -0.0
            m[s:s + 8] = -0.0
            p[s:s + 8] = -0.0
            r_dev.copy_(r_ref)
            m_dev.copy_(m)
            p_dev.copy_(p)
        kw = None if mom is None else dict(exp_avg=m, beta1=0.9, weight_decay=mom, param=p)
        kd = None if mom is None else dict(exp_avg=m_dev, beta1=0.9, weight_decay=mom, param=p_dev)
        g_dev = g.to(DEV)
        cpu.ts_encode(0, g, rows_ref, r_ref, kw)
        gpu.ts_encode(0, g_dev, rows_dev, r_dev, kd)
        got = rows_dev.cpu()
        assert torch.equal(got, rows_ref), \
            f"push {it}: rows differ at {(got != rows_ref).nonzero()[:8].tolist()}"
        assert _bits(r_dev, r_ref), f"push {it}: worker residual"
        assert _bits(g_dev, g) and _bits(m_dev, m) and _bits(p_dev, p)  # only read
        a, w = ts.slots[2]  # the all-zero chunk: scale 0 and no bit, then a real scale
        zero = int(rows_ref.view(-1)[a:a + 4].view(torch.int32)) == 0
        assert zero == (it == 0)
        assert it == 1 or int(rows_ref.view(-1)[w:w + 1024].abs().max()) == 0


@pytest.mark.parametrize("nranks", [1, 2, 3, 8])
@pytest.mark.parametrize("shards", [1, 2, 3])
def test_owner_reduce_encode_matches_oracle(shards, nranks):
    ops.require()
    ts, cpu, gpu = _pair(shards)
    stride = ts.P + 32  # strictly larger than every shard's payload
    for o, (s0, ln, sp, lay, _) in enumerate(ts.shards):
        assert stride > lay.nbytes
        recv = torch.zeros((nranks, stride), dtype=torch.uint8)
        for r in range(nranks):  # very different magnitudes per rank: the sum's order matters
            recv[r, :lay.nbytes] = oracle.encode_sign(
                _vec(sp, 100 + 10 * o + r, 3.0 ** r), sp, lay, None)
        recv[-1, lay.scales:lay.scales + 4] = 0  # the last rank's first chunk: scale 0
        sres = torch.zeros(ts.max_shard)
        sres[:ln] = _vec(sp, 200 + o, 0.05)
        # a chunk whose mean + server residual is exactly 0: scale 0, no bit, residual 0
        last = sp.num_chunks - 1
        cs, cl = sp.chunk_start[last], sp.chunk_len[last]
        mean = oracle.decode_sum(recv[:, :lay.nbytes].contiguous(), sp, lay, 0, 1.0 / nranks)
        sres[cs:cs + cl] = -mean[cs:cs + cl]
        s_dev, recv_dev = sres.to(DEV), recv.to(DEV)
        own_ref = torch.zeros(ts.P, dtype=torch.uint8)
        own_dev = torch.zeros(ts.P, dtype=torch.uint8, device=DEV)
        for it in range(2):
            cpu.ts_reduce_encode(0, o, recv, own_ref, 1.0 / nranks, sres)
            gpu.ts_reduce_encode(0, o, recv_dev, own_dev, 1.0 / nranks, s_dev)
            got = own_dev.cpu()
            assert torch.equal(got, own_ref), \
                f"shard {o} call {it}: differs at {(got != own_ref).nonzero()[:8].flatten()}"
            assert _bits(s_dev, sres), f"shard {o} call {it}: server residual"
            assert torch.equal(recv_dev.cpu(), recv)  # only read
            if it == 0:
                sc = own_ref[lay.scales + 4 * last:lay.scales + 4 * last + 4].view(torch.float32)
                assert float(sc) == 0.0
                assert int(own_ref[lay.codes + 1024 * last:lay.codes + 1024 * last + 1024]
                           .abs().max()) == 0


def test_owner_kernel_in_a_graph_equals_eager():
    ops.require()
    ts, _, gpu = _pair(2)
    _, ln, sp, lay, _ = ts.shards[1]
    recv = torch.zeros((3, ts.P), dtype=torch.uint8)
    for r in range(3):
        recv[r, :lay.nbytes] = oracle.encode_sign(_vec(sp, 300 + r), sp, lay, None)
    recv = recv.to(DEV)
    s0 = torch.zeros(ts.max_shard)
    s0[:ln] = _vec(sp, 310, 0.05)
    s_eager, s_graph = s0.to(DEV), s0.to(DEV)
    own_eager = torch.zeros(ts.P, dtype=torch.uint8, device=DEV)
    own_graph = torch.zeros(ts.P, dtype=torch.uint8, device=DEV)
    first = []
    for _ in range(2):
        gpu.ts_reduce_encode(0, 1, recv, own_eager, 1.0 / 3, s_eager)
        first.append(own_eager.clone())
    assert not torch.equal(first[0], first[1])  # the residual moved the second payload
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph(keep_graph=True)
    with torch.cuda.graph(g, capture_error_mode="thread_local"):
        gpu.ts_reduce_encode(0, 1, recv, own_graph, 1.0 / 3, s_graph)
    info = ops.graph_info(g.raw_cuda_graph())
    assert info["linear"] and info["types"] == {"kernel": 1}
    g.instantiate()
    for i in range(2):
        g.replay()
        torch.cuda.synchronize()
        assert torch.equal(own_graph, first[i]), f"replay {i}"
    assert _bits(s_graph, s_eager)


@pytest.mark.parametrize("momentum", [0.5, 0.0])
@pytest.mark.parametrize("shards", [1, 2, 3])
def test_pull_decode_sgd_matches_oracle(pushed, shards, momentum):
    ops.require()
    ts, cpu, gpu = _pair(shards)
    plan = ts.plan
    rows = pushed[shards]
    rows_dev = rows.to(DEV)
    hp = dict(HP, momentum=momentum)
    p_ref, b_ref = _vec(plan, 1), _vec(plan, 2, 0.1)
    p_dev, b_dev = p_ref.to(DEV), b_ref.to(DEV)
    sh = torch.zeros(plan.length, dtype=torch.bfloat16, device=DEV)
    go_ref, go_dev = torch.zeros(plan.length), torch.zeros(plan.length, device=DEV)
    for first in (True, False):
        mom_ref, mom_dev = (b_ref, b_dev) if momentum else (None, None)
        cpu.ts_decode_apply_sgd(0, rows, p_ref, mom_ref, hp, first, grad_out=go_ref)
        gpu.ts_decode_apply_sgd(0, rows_dev, p_dev, mom_dev, hp, first, grad_out=go_dev,
                                shadow=sh)
        assert _bits(go_dev, go_ref), "decoded mean"
        assert _bits(p_dev, p_ref), "parameters"
        assert _bits(b_dev, b_ref), "momentum"
        for off, n in zip(plan.offsets, plan.numels):
            assert torch.equal(sh[off:off + n].cpu(), p_ref[off:off + n].to(torch.bfloat16))
    # decode only (an optimizer without a fused step)
    go_dev.zero_()
    gpu.ts_decode_apply_sgd(0, rows_dev, None, None, None, False, grad_out=go_dev)
    assert _bits(go_dev, go_ref)
    assert torch.equal(rows_dev.cpu(), rows)


@pytest.mark.parametrize("shards", [1, 2, 3])
def test_pull_decode_onebit_matches_oracle(pushed, shards):
    ops.require()
    ts, cpu, gpu = _pair(shards)
    plan = ts.plan
    rows = pushed[shards]
    rows_dev = rows.to(DEV)
    p_ref, v = _vec(plan, 1), _vec(plan, 3).square()
    v[plan.offsets[2]:plan.offsets[2] + 100] = 0.0  # never saw a gradient: parameter kept
    m_ref = torch.zeros(plan.length)
    p_dev, v_dev, m_dev = p_ref.to(DEV), v.to(DEV), m_ref.to(DEV)
    sh = torch.zeros(plan.length, dtype=torch.bfloat16, device=DEV)
    hp = dict(lr=1e-3, lr_step=oracle.onebit_lr_step(1e-3, 0.9, 0.999, 7, 4), betas=(0.9, 0.999),
              eps=1e-8, freeze_step=4)
    before = p_ref.clone()
    cpu.ts_decode_apply_onebit(0, rows, p_ref, m_ref, v, hp)
    gpu.ts_decode_apply_onebit(0, rows_dev, p_dev, m_dev, v_dev, hp, shadow=sh)
    assert _bits(m_dev, m_ref), "exp_avg"
    assert _bits(p_dev, p_ref), "parameters"
    assert _bits(v_dev, v)
    assert not _bits(p_ref, before)
    for off, n in zip(plan.offsets, plan.numels):
        assert torch.equal(sh[off:off + n].cpu(), p_ref[off:off + n].to(torch.bfloat16))
    # the device step counter gives the same lr_step to fp32
    p2, m2 = before.to(DEV), torch.zeros(plan.length, device=DEV)
    step = torch.full((1,), 6, dtype=torch.int32, device=DEV)
    gpu.ts_decode_apply_onebit(0, rows_dev, p2, m2, v_dev, dict(hp, lr_step=0.0, step_t=step))
    assert _bits(m2, m_ref)
    torch.testing.assert_close(p2.cpu(), p_ref, rtol=1e-6, atol=1e-9)


def test_wrapper_refusals_raise_before_any_launch():
    ops.require()
    ts, _, gpu = _pair(3)
    sl = gpu.ts_dev[0]
    plan = ts.plan
    g = torch.zeros(plan.length, device=DEV)
    r = torch.zeros(plan.length, device=DEV)
    rows = torch.zeros((ts.N, ts.P), dtype=torch.uint8, device=DEV)
    other = ops.SignSlots(TwoStagePlan(_plan(), shard_plans(_plan(), 2, 0)), DEV)
    with pytest.raises(ValueError, match="same bucket"):
        ops.sign_encode(sl, g, rows, None, r, slots=other)
    with pytest.raises(ValueError, match="bytes"):
        ops.sign_encode(sl, g, rows.view(-1)[:-16], None, r, slots=sl)
    with pytest.raises(TypeError):
        ops.sign_encode(sl, g, rows.view(torch.int8), None, r, slots=sl)
    with pytest.raises(ValueError, match="aligned"):
        ops.sign_decode_apply(sl, torch.zeros(ts.N * ts.P + 16, dtype=torch.uint8,
                                              device=DEV)[4:], None, grad_out=g, slots=sl)
    with pytest.raises(ValueError, match="elements"):
        ops.sign_decode_apply(sl, rows, None, grad_out=g[:-64], slots=sl)
    with pytest.raises(ValueError, match="1-bit Adam step needs"):
        ops.sign_decode_onebit(sl, rows, None, g, None, g, 1.0, 0.1, 1e-8, slots=sl)
    _, ln, sp, lay, _ = ts.shards[1]
    st = gpu.ts_shard_dev[0][1]
    sres = torch.zeros(ts.max_shard, device=DEV)
    own = torch.zeros(ts.P, dtype=torch.uint8, device=DEV)
    with pytest.raises(ValueError, match="row stride"):
        ops.sign_reduce_encode(st, torch.zeros((2, lay.nbytes - 16), dtype=torch.uint8,
                                               device=DEV), lay, 0.5, sres, own)
    with pytest.raises(TypeError):
        ops.sign_reduce_encode(st, rows.view(torch.int8), lay, 0.5, sres, own)
    with pytest.raises(ValueError, match="out too small"):
        ops.sign_reduce_encode(st, rows, lay, 0.5, sres, own[:lay.nbytes - 16])
    with pytest.raises(ValueError, match="elements"):
        ops.sign_reduce_encode(st, rows, lay, 0.5, sres[:ln - 64], own)
    with pytest.raises(ValueError, match="server residual"):
        ops.sign_reduce_encode(st, rows, lay, 0.5, None, own)
    with pytest.raises(ValueError, match="nranks"):
        ops.sign_reduce_encode(st, torch.zeros((65, ts.P), dtype=torch.uint8, device=DEV), lay,
                               0.5, sres, own)
    with pytest.raises(ValueError, match="128"):
        TwoStagePlan(_plan([64] * 129), shard_plans(_plan([64] * 129), 2, 0))
    torch.cuda.synchronize()
    assert int(rows.abs().max()) == 0 and int(own.abs().max()) == 0  # nothing ran
