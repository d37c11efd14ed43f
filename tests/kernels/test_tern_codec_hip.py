"""The TernGrad codec's HIP kernels (ops/csrc/tern_codec.hip) vs the torch oracle, on one MI355X.

Exactness contract: payload bytes (scalers, 2-bit codes, zero pad codes and the alignment pads),
residuals, decoded sums, the fused SGD step and the key advance are bitwise the oracle's, on the
bucket of edge-case tensors that the CPU tests share (tests/tern_sim.py)."""
import pytest
import torch

from ewdml import ops
from ewdml.compress import oracle
from ewdml.compress.plan import BucketPlan, Layout
from ewdml.compress.rng import stream_key
from tests import tern_sim as sim

pytestmark = pytest.mark.gpu

DEV = "cuda"
CLIPS = [0.0, 2.5]
SEED = 3


def _plan(numels=sim.NUMELS, bucket_offset=sim.BUCKET_OFFSET):
    offs, length = sim.offsets(numels)
    return BucketPlan(list(numels), offs, 1.0, bucket_offset, length)


def _bucket(seed):
    return torch.from_numpy(sim.bucket(seed))


def _bits(t):
    return t.contiguous().view(torch.int32)


def _scales(pay, plan, lay):
    return oracle._section(pay, lay.scales, plan.num_tensors, torch.float32)


@pytest.mark.parametrize("clip", CLIPS)
@pytest.mark.parametrize("ef", [False, True], ids=["plain", "ef"])
def test_encode_matches_oracle(ef, clip):
    """Two encodes into the same buffers (the second with the next step's key and another
    gradient: a stale pad, max key or partial sum would show), the payload pre-filled with 0xFF so
    that an unwritten byte shows."""
    ops.require()
    plan = _plan()
    lay = Layout.build("tern", plan)
    dp = ops.DevicePlan(plan, DEV)
    pay = torch.full((lay.nbytes,), 0xFF, dtype=torch.uint8, device=DEV)
    r_ref = _bucket(1) * 0.25 if ef else None
    r_dev = r_ref.to(DEV) if ef else None
    for it in range(2):
        g = _bucket(2 * it)
        key = stream_key(SEED, 7 + it, 1)
        ref = oracle.encode_tern(g.clone(), plan, lay, clip, key, r_ref)
        ops.tern_encode(dp, g.to(DEV), pay, lay, clip, key, resid=r_dev)
        got = pay.cpu()
        sg, sr = _scales(got, plan, lay), _scales(ref, plan, lay)
        assert torch.equal(_bits(sg), _bits(sr)), f"encode {it}: scalers {sg} vs {sr}"
        assert torch.equal(got, ref), \
            f"encode {it}: payload differs at {(got != ref).nonzero()[:10].flatten()}"
        if ef:
            assert torch.equal(_bits(r_dev.cpu()), _bits(r_ref)), f"encode {it}: residual"
    # the shared bucket does what it is for: a zero scaler, an unclipped constant, a clipped outlier
    assert sr[sim.ZERO_T] == 0 and sr[0] > 0
    if clip > 0 and not ef:
        assert sr[sim.OUTLIER_T] < 0.1 * sim.OUTLIER and sr[sim.CONST_T] == 0.375


def test_sum_order_across_many_chunks():
    """A tensor of more than 256 chunks: the scale kernel's threads add several partials each
    before the tree, as oracle._tern_sumsq does.  Clipped, so the scaler is the sum's."""
    ops.require()
    plan = _plan([300 * 8192 + 77, 5])
    lay = Layout.build("tern", plan)
    dp = ops.DevicePlan(plan, DEV)
    g = torch.zeros(plan.length)
    gen = torch.Generator().manual_seed(21)
    g[:plan.numels[0]] = torch.randn(plan.numels[0], generator=gen)
    g[plan.offsets[1]:plan.offsets[1] + 5] = torch.randn(5, generator=gen)
    pay = torch.full((lay.nbytes,), 0xFF, dtype=torch.uint8, device=DEV)
    key = stream_key(SEED, 1, 0)
    ops.tern_encode(dp, g.to(DEV), pay, lay, 2.5, key)
    ref = oracle.encode_tern(g, plan, lay, 2.5, key)
    got = pay.cpu()
    assert torch.equal(_bits(_scales(got, plan, lay)), _bits(_scales(ref, plan, lay)))
    assert _scales(ref, plan, lay)[0] < g.abs().max()
    assert torch.equal(got, ref)


@pytest.mark.parametrize("ef", [False, True], ids=["plain", "ef"])
def test_key_from_device_memory(ef):
    ops.require()
    plan = _plan()
    lay = Layout.build("tern", plan)
    dp = ops.DevicePlan(plan, DEV)
    g = _bucket(0).to(DEV)
    key = stream_key(SEED, 12, 2)
    ks = torch.tensor([12, key - (1 << 32) if key >= 1 << 31 else key], dtype=torch.int32,
                      device=DEV)
    out = []
    for kw in (dict(key=key), dict(key=0x5A5A5A5A, key_tensor=ks[1:2])):  # the device key wins
        pay = torch.full((lay.nbytes,), 0xFF, dtype=torch.uint8, device=DEV)
        r = (_bucket(1) * 0.25).to(DEV) if ef else None
        ops.tern_encode(dp, g, pay, lay, 2.5, resid=r, **kw)
        out.append((pay.cpu(), None if r is None else r.cpu()))
    assert torch.equal(out[0][0], out[1][0])
    assert torch.equal(out[0][0], oracle.encode_tern(_bucket(0), plan, lay, 2.5, key,
                                                     _bucket(1) * 0.25 if ef else None))
    if ef:
        assert torch.equal(_bits(out[0][1]), _bits(out[1][1]))


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_encode_from_per_tensor_pointers(dtype):
    """Autograd's own per-tensor gradients (fp32 or bf16, read through the pointer table) give the
    flat form's payload, with and without the residual; the gradients are not modified."""
    ops.require()
    plan = _plan()
    lay = Layout.build("tern", plan)
    g = _bucket(0)
    for o, n in zip(plan.offsets, plan.numels):  # the flat reference holds the same values
        g[o:o + n] = g[o:o + n].to(dtype).float()
    dp = ops.DevicePlan(plan, DEV)
    grads = [g[o:o + n].clone().to(dtype).to(DEV) for o, n in zip(plan.offsets, plan.numels)]
    before = [t.clone() for t in grads]
    key = stream_key(SEED, 2, 0)
    pay = torch.full((lay.nbytes,), 0xFF, dtype=torch.uint8, device=DEV)
    flat = torch.full((lay.nbytes,), 0xFF, dtype=torch.uint8, device=DEV)
    ops.tern_encode(dp, grads, pay, lay, 2.5, key)
    ops.tern_encode(dp, g.to(DEV), flat, lay, 2.5, key)
    assert torch.equal(pay, flat)
    assert torch.equal(pay.cpu(), oracle.encode_tern(g.clone(), plan, lay, 2.5, key))
    r_ref = _bucket(1) * 0.25
    r_dev = r_ref.to(DEV)
    ref = oracle.encode_tern(g.clone(), plan, lay, 2.5, key, r_ref)
    ops.tern_encode(dp, grads, pay, lay, 2.5, key, resid=r_dev)
    assert torch.equal(pay.cpu(), ref)
    assert torch.equal(_bits(r_dev.cpu()), _bits(r_ref))
    for a, b in zip(grads, before):
        assert torch.equal(a, b)


# ---- decode ---------------------------------------------------------------------------------------
_DECODED = {}


def _rows(N):
    """(plan, layout, received rows, their decoded mean), computed once per N and only read.  The
    ranks' gradients differ in magnitude, so the rank order of the fp32 sum matters."""
    if N not in _DECODED:
        plan = _plan()
        lay = Layout.build("tern", plan)
        recv = torch.stack([oracle.encode_tern(_bucket(10 + r) * (3.0 ** (r % 4)), plan, lay,
                                               2.5 if r % 2 else 0.0, stream_key(SEED, 5, r))
                            for r in range(N)])
        _DECODED[N] = (plan, lay, recv, oracle.decode_sum(recv, plan, lay, 1, 1.0 / N))
    return _DECODED[N]


@pytest.mark.parametrize("N", [1, 2, 3, 8])
def test_decode_grad_out(N):
    ops.require()
    plan, lay, recv, g = _rows(N)
    dp = ops.DevicePlan(plan, DEV)
    go = torch.full((plan.length,), float("nan"), device=DEV)
    ops.tern_decode_apply(dp, recv.to(DEV), lay, grad_out=go, grad_scale=1.0 / N)
    got = go.cpu()
    own = torch.zeros(plan.length, dtype=torch.bool)
    for off, n in zip(plan.offsets, plan.numels):
        own[off:off + n] = True
    assert torch.equal(_bits(got[own]), _bits(g[own]))
    assert torch.isnan(got[~own]).all()  # nothing is written between the tensors
    assert g[own].abs().max() > 0


# lr = 2^-4 and dampening = 0: lr * d and (1 - dampening) * d are exact, so the reference does not
# depend on whether torch's CPU ``add_(x, alpha=)`` contracts its multiply-add (the kernels never
# do); every other step of oracle.sgd_apply is a separately rounded operation
HP = dict(lr=0.0625, momentum=0.9, dampening=0.0, weight_decay=5e-4)


@pytest.mark.parametrize("first", [True, False], ids=["first", "later"])
@pytest.mark.parametrize("nesterov", [True, False], ids=["nesterov", "heavy-ball"])
@pytest.mark.parametrize("N", [1, 2, 3, 8])
def test_decode_apply_sgd(N, nesterov, first):
    ops.require()
    plan, lay, recv, g = _rows(N)
    hp = dict(HP, nesterov=nesterov)
    gen = torch.Generator().manual_seed(11)
    p0 = torch.randn(plan.length, generator=gen)
    m0 = torch.randn(plan.length, generator=gen)
    p, m = p0.clone(), m0.clone()
    for off, n in zip(plan.offsets, plan.numels):
        oracle.sgd_apply(p[off:off + n], m[off:off + n], g[off:off + n], first=first, **hp)
    dp = ops.DevicePlan(plan, DEV)
    pd, md = p0.to(DEV), m0.to(DEV)
    sh = torch.zeros(plan.length, dtype=torch.bfloat16, device=DEV)
    seed, step, rank = 5, 41, 3
    ks = torch.tensor([step, 0], dtype=torch.int32, device=DEV)
    lr_t = torch.tensor([hp["lr"]], device=DEV)  # the device scalar wins over the host value
    ops.tern_decode_apply(dp, recv.to(DEV), lay, param=pd, mom=md, grad_scale=1.0 / N,
                          first=first, shadow=sh, key_state=ks, key_seed=seed, key_rank=rank,
                          lr_tensor=lr_t, **dict(hp, lr=999.0))
    assert torch.equal(_bits(pd.cpu()), _bits(p))  # the positions between tensors included
    assert torch.equal(_bits(md.cpu()), _bits(m))
    for off, n in zip(plan.offsets, plan.numels):
        assert torch.equal(sh[off:off + n].cpu(), p[off:off + n].to(torch.bfloat16))
    assert [int(v) & 0xFFFFFFFF for v in ks.cpu()] == [step + 1, stream_key(seed, step + 1, rank)]


def test_decode_apply_without_momentum():
    ops.require()
    plan, lay, recv, g = _rows(2)
    hp = dict(lr=0.0625, momentum=0.0, dampening=0.0, weight_decay=0.0, nesterov=False)
    p0 = torch.randn(plan.length, generator=torch.Generator().manual_seed(12))
    p = p0.clone()
    for off, n in zip(plan.offsets, plan.numels):
        oracle.sgd_apply(p[off:off + n], None, g[off:off + n], first=False, **hp)
    pd = p0.to(DEV)
    ops.tern_decode_apply(ops.DevicePlan(plan, DEV), recv.to(DEV), lay, param=pd, mom=None,
                          grad_scale=0.5, **hp)
    assert torch.equal(_bits(pd.cpu()), _bits(p))


def test_encode_decode_graph_capture():
    """Encode (key from device memory) + decode-apply (key advance) captured on one stream and
    replayed with fresh gradients copied into the static buffer: bitwise the eager run with host
    keys."""
    ops.require()
    plan = _plan([8192 * 2 + 5, 700, 3])
    lay = Layout.build("tern", plan)
    dp = ops.DevicePlan(plan, DEV)
    hp = dict(lr=0.05, momentum=0.9, dampening=0.0, weight_decay=1e-4, nesterov=False)
    gen = torch.Generator().manual_seed(60)
    grads = [(torch.randn(plan.length, generator=gen) * 0.1).to(DEV) for _ in range(3)]
    p0 = torch.randn(plan.length, generator=gen).to(DEV)

    def state():
        return dict(g=torch.zeros(plan.length, device=DEV), r=torch.zeros(plan.length, device=DEV),
                    p=p0.clone(), m=torch.zeros(plan.length, device=DEV),
                    pay=torch.zeros(1, lay.nbytes, dtype=torch.uint8, device=DEV))

    eager = state()
    for i, g in enumerate(grads):
        eager["g"].copy_(g)
        ops.tern_encode(dp, eager["g"], eager["pay"][0], lay, 2.5, stream_key(SEED, 1 + i, 0),
                        resid=eager["r"])
        ops.tern_decode_apply(dp, eager["pay"], lay, param=eager["p"], mom=eager["m"],
                              first=False, **hp)
    cap = state()
    k1 = stream_key(SEED, 1, 0)
    ks = torch.tensor([1, k1 - (1 << 32) if k1 >= 1 << 31 else k1], dtype=torch.int32, device=DEV)
    cap["g"].copy_(grads[0])
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        with torch.cuda.graph(graph, stream=side):
            ops.tern_encode(dp, cap["g"], cap["pay"][0], lay, 2.5, 0, resid=cap["r"],
                            key_tensor=ks[1:2])
            ops.tern_decode_apply(dp, cap["pay"], lay, param=cap["p"], mom=cap["m"], first=False,
                                  key_state=ks, key_seed=SEED, key_rank=0, **hp)
    torch.cuda.current_stream().wait_stream(side)
    graph.replay()  # capturing does not run: this is the first step
    for g in grads[1:]:
        cap["g"].copy_(g)
        graph.replay()
    torch.cuda.synchronize()
    for k in ("p", "m", "r", "pay"):
        assert torch.equal(cap[k], eager[k]), k
    assert eager["r"].abs().max() > 0 and int(ks[0]) == 4


def test_bad_operands_rejected():
    """Size, dtype, alignment and the layout are checked on the host, before any launch."""
    ops.require()
    plan = _plan([1000, 8192 + 1])
    lay = Layout.build("tern", plan)
    dp = ops.DevicePlan(plan, DEV)
    g = torch.zeros(plan.length, device=DEV)
    pay = torch.zeros(lay.nbytes, dtype=torch.uint8, device=DEV)
    bigpay = torch.zeros(lay.nbytes + 16, dtype=torch.uint8, device=DEV)
    big = torch.zeros(plan.length + 4, device=DEV)
    with pytest.raises(ValueError):  # payload too short
        ops.tern_encode(dp, g, pay[:lay.nbytes - 16], lay, 2.5, 1)
    with pytest.raises(ValueError):  # gradient too short
        ops.tern_encode(dp, g[:100], pay, lay, 2.5, 1)
    with pytest.raises(TypeError):
        ops.tern_encode(dp, g.double(), pay, lay, 2.5, 1)
    with pytest.raises(TypeError):
        ops.tern_encode(dp, g, pay, lay, 2.5, 1, resid=g.to(torch.bfloat16))
    with pytest.raises(ValueError):  # misaligned views
        ops.tern_encode(dp, g, bigpay[4:], lay, 2.5, 1)
    with pytest.raises(ValueError):
        ops.tern_encode(dp, g, pay, lay, 2.5, 1, resid=big[1:])
    with pytest.raises(ValueError):  # a negative clip
        ops.tern_encode(dp, g, pay, lay, -1.0, 1)
    with pytest.raises(ValueError):  # another codec's layout, another plan's layout
        ops.tern_encode(dp, g, pay, Layout.build("qsgd", plan, 4), 2.5, 1)
    with pytest.raises(ValueError):
        ops.tern_encode(dp, g, pay, Layout.build("tern", _plan([1000, 8192 + 1, 64])), 2.5, 1)
    with pytest.raises(ValueError):  # row length is not the layout's
        ops.tern_decode_apply(dp, bigpay[None], lay, grad_out=g)
    with pytest.raises(ValueError):  # nothing to do
        ops.tern_decode_apply(dp, pay[None], lay)
    with pytest.raises(ValueError):
        ops.tern_decode_apply(dp, pay[None], lay, param=g, mom=None, lr=0.0625, momentum=0.9)
    torch.cuda.synchronize()
    assert not pay.any() and not g.any()  # nothing ran
