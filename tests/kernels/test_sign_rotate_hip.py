"""The Hadamard-rotated sign codec's HIP kernels (ops/csrc/sign_codec.hip k_hsign_encode /
k_hsign_decode_apply) vs the torch oracle, on one MI355X.

Exactness contract: payload bytes, residuals, decoded sums and the fused SGD step are bitwise the
oracle's.  The transform's 13 butterfly stages run in ``oracle.HSIGN_STAGE_BITS`` order, every
butterfly is one separately rounded fp32 add, and the file set is built with -ffp-contract=off.
"""
import pytest
import torch

from ewdml import ops
from ewdml.compress import oracle
from ewdml.compress.plan import BucketPlan, Layout
from ewdml.compress.rng import stream_key

pytestmark = pytest.mark.gpu

DEV = "cuda"
KEY = oracle.hsign_rot_key(3, 1)

# one-element tensor and a tail shorter than a word | tails of 1..5 | a 5-element tail after full
# chunks, multi-chunk tensors
SHAPES = [[10], [1, 2, 3, 4, 5], [500, 10], [8192 * 3 + 5, 7, 64, 100003]]


def _plan(numels, bucket_offset=4096):
    offs, o = [], 0
    for n in numels:
        offs.append(o)
        o += (n + 63) // 64 * 64
    return BucketPlan(numels, offs, 1.0, bucket_offset, o)


def _grad(plan, seed=0):
    g = torch.zeros(plan.length)
    gen = torch.Generator().manual_seed(seed)
    for off, n in zip(plan.offsets, plan.numels):
        g[off:off + n] = torch.randn(n, generator=gen) * (0.1 + torch.rand(1, generator=gen))
    return g


def _bits_equal(a, b):
    """Bitwise equality of fp32 tensors (tells -0.0 from +0.0, compares NaN payloads)."""
    return torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def _split(plan, g, dtype=torch.float32):
    return [g[o:o + n].clone().to(dtype).to(DEV) for o, n in zip(plan.offsets, plan.numels)]


@pytest.mark.parametrize("ef", [False, True])
@pytest.mark.parametrize("numels", SHAPES)
def test_encode_matches_oracle(numels, ef):
    ops.require()
    plan = _plan(numels)
    lay = Layout.build("sign", plan)
    dp = ops.DevicePlan(plan, DEV)
    pay = torch.full((lay.nbytes,), 0xFF, dtype=torch.uint8, device=DEV)  # padding is rewritten
    r_ref = _grad(plan, seed=50) * 0.3 if ef else None
    r_dev = r_ref.to(DEV) if ef else None
    for it in range(2):
        g = _grad(plan, seed=len(numels) + it)
        ref = oracle.encode_sign(g.clone(), plan, lay, r_ref, KEY)
        ops.sign_encode(dp, g.to(DEV), pay, lay, resid=r_dev, rot_key=KEY)
        got = pay.cpu()
        assert torch.equal(got, ref), \
            f"encode {it}: payload differs at {(got != ref).nonzero()[:10].flatten()}"
        if ef:
            assert _bits_equal(r_dev.cpu(), r_ref), f"encode {it}: residual"
    assert not torch.equal(ref, oracle.encode_sign(g.clone(), plan, lay))  # it is rotated


def test_encode_zero_chunk_and_one_hot():
    ops.require()
    plan = _plan([8192 + 300, 100])
    lay = Layout.build("sign", plan)
    dp = ops.DevicePlan(plan, DEV)
    r_dev = torch.zeros(plan.length, device=DEV)
    pay = torch.full((lay.nbytes,), 0xFF, dtype=torch.uint8, device=DEV)
    ops.sign_encode(dp, torch.zeros(plan.length, device=DEV), pay, lay, resid=r_dev, rot_key=KEY)
    assert torch.equal(pay.cpu(), oracle.encode_sign(torch.zeros(plan.length), plan, lay,
                                                     torch.zeros(plan.length), KEY))
    assert not pay[lay.scales:lay.codes].any() and not r_dev.any()  # scale 0, residual stays 0
    g = torch.zeros(plan.length)
    g[4321] = -3.5
    r_ref = torch.zeros(plan.length)
    ref = oracle.encode_sign(g.clone(), plan, lay, r_ref, KEY)
    ops.sign_encode(dp, g.to(DEV), pay, lay, resid=r_dev, rot_key=KEY)
    assert torch.equal(pay.cpu(), ref) and _bits_equal(r_dev.cpu(), r_ref)
    out = torch.zeros(plan.length, device=DEV)
    ops.sign_decode_apply(dp, pay[None], lay, grad_out=out, rot_key=KEY)
    assert torch.equal(out.cpu(), g)  # a one-hot chunk reconstructs exactly


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_encode_from_per_tensor_pointers(dtype):
    """Autograd's own per-tensor gradients (fp32 or bf16, read through the pointer table), with
    the error feedback staged in the fp32 residual; the gradients are not modified."""
    ops.require()
    plan = _plan([8192 + 7, 64, 30000, 5], bucket_offset=256)
    lay = Layout.build("sign", plan)
    g = _grad(plan, seed=3)
    for o, n in zip(plan.offsets, plan.numels):  # the flat reference holds the same values
        g[o:o + n] = g[o:o + n].to(dtype).float()
    dp = ops.DevicePlan(plan, DEV)
    pay = torch.zeros(lay.nbytes, dtype=torch.uint8, device=DEV)
    grads = _split(plan, g, dtype)
    before = [t.clone() for t in grads]
    ops.sign_encode(dp, grads, pay, lay, rot_key=KEY)
    assert torch.equal(pay.cpu(), oracle.encode_sign(g.clone(), plan, lay, None, KEY))
    r_ref = _grad(plan, seed=8) * 0.05
    r_dev = r_ref.to(DEV)
    ref = oracle.encode_sign(g.clone(), plan, lay, r_ref, KEY)
    ops.sign_encode(dp, grads, pay, lay, resid=r_dev, rot_key=KEY)
    assert torch.equal(pay.cpu(), ref)
    assert _bits_equal(r_dev.cpu(), r_ref)
    for a, b in zip(grads, before):
        assert torch.equal(a, b)


def _payloads(plan, lay, N, seed=100):
    # very different magnitudes per rank: the rank order of the fp32 sum matters
    return torch.stack([oracle.encode_sign(_grad(plan, seed=seed + r) * (3.0 ** r), plan, lay,
                                           None, KEY) for r in range(N)])


@pytest.mark.parametrize("N", [1, 2, 4, 11])
def test_decode_matches_oracle(N):
    ops.require()
    plan = _plan([20 * 25, 20, 8192 * 2 + 3, 1, 70001], bucket_offset=128)
    lay = Layout.build("sign", plan)
    recv = _payloads(plan, lay, N)
    ref = oracle.decode_sum(recv, plan, lay, 127, 1.0 / N, KEY)
    dp = ops.DevicePlan(plan, DEV)
    out = torch.full((plan.length,), float("nan"), device=DEV)
    ops.sign_decode_apply(dp, recv.to(DEV), lay, grad_out=out, grad_scale=1.0 / N, rot_key=KEY)
    got = out.cpu()
    for off, n in zip(plan.offsets, plan.numels):
        assert _bits_equal(got[off:off + n], ref[off:off + n])
    gaps = torch.ones(plan.length, dtype=torch.bool)
    for off, n in zip(plan.offsets, plan.numels):
        gaps[off:off + n] = False
    assert torch.isnan(got[gaps]).all()  # nothing is written between the tensors


# lr = 2^-4 and dampening = 0: lr * d and (1 - dampening) * d are exact, so the reference's
# result does not depend on whether torch's CPU ``add_(x, alpha=)`` contracts its multiply-add
# (the kernels never do); every other step of oracle.sgd_apply is a separately rounded operation
@pytest.mark.parametrize("hp,first,with_mom", [
    (dict(lr=0.0625, momentum=0.9, dampening=0.0, weight_decay=0.0, nesterov=False), True, True),
    (dict(lr=0.0625, momentum=0.9, dampening=0.0, weight_decay=0.0, nesterov=False), False, True),
    (dict(lr=0.0625, momentum=0.9, dampening=0.0, weight_decay=5e-4, nesterov=True), False, True),
    (dict(lr=0.0625, momentum=0.0, dampening=0.0, weight_decay=0.0, nesterov=False), False, False),
])
def test_decode_fused_sgd_bitwise(hp, first, with_mom):
    ops.require()
    plan = _plan([9000, 64, 33333, 3])
    lay = Layout.build("sign", plan)
    N = 3
    recv = _payloads(plan, lay, N, seed=7)
    g = oracle.decode_sum(recv, plan, lay, 127, 1.0 / N, KEY)
    gen = torch.Generator().manual_seed(11)
    p0 = torch.randn(plan.length, generator=gen)
    m0 = torch.randn(plan.length, generator=gen)
    p, m = p0.clone(), m0.clone()
    for off, n in zip(plan.offsets, plan.numels):
        oracle.sgd_apply(p[off:off + n], m[off:off + n] if with_mom else None, g[off:off + n],
                         first=first, **hp)
    dp = ops.DevicePlan(plan, DEV)
    pd, md = p0.to(DEV), m0.to(DEV)
    go = torch.zeros(plan.length, device=DEV)
    ops.sign_decode_apply(dp, recv.to(DEV), lay, param=pd, mom=md if with_mom else None,
                          grad_out=go, grad_scale=1.0 / N, first=first, rot_key=KEY, **hp)
    assert _bits_equal(pd.cpu(), p)
    assert _bits_equal(md.cpu(), m)  # untouched when with_mom is False
    for off, n in zip(plan.offsets, plan.numels):
        assert _bits_equal(go.cpu()[off:off + n], g[off:off + n])


def test_decode_shadow_and_key_state():
    ops.require()
    plan = _plan([9000, 64, 33333])
    lay = Layout.build("sign", plan)
    recv = _payloads(plan, lay, 2).to(DEV)
    dp = ops.DevicePlan(plan, DEV)
    p = torch.randn(plan.length, device=DEV)
    m = torch.zeros(plan.length, device=DEV)
    sh = torch.zeros(plan.length, dtype=torch.bfloat16, device=DEV)
    seed, step, rank = 5, 41, 3
    ks = torch.tensor([step, 0], dtype=torch.int32, device=DEV)
    ops.sign_decode_apply(dp, recv, lay, param=p, mom=m, lr=0.1, momentum=0.9, grad_scale=0.5,
                          first=True, shadow=sh, key_state=ks, key_seed=seed, key_rank=rank,
                          rot_key=KEY)
    for o, n in zip(plan.offsets, plan.numels):
        assert torch.equal(sh[o:o + n], p[o:o + n].to(torch.bfloat16))
    got = [int(v) & 0xFFFFFFFF for v in ks.cpu()]
    assert got == [step + 1, stream_key(seed, step + 1, rank)]


def test_encode_decode_graph_capture():
    """Encode + decode-apply captured on one stream and replayed with fresh gradients copied into
    the static buffers: bitwise the eager run (the rotation key is a constant of the bucket, so
    the graph takes no new input)."""
    ops.require()
    plan = _plan([8192 * 2 + 5, 700, 3])
    lay = Layout.build("sign", plan)
    dp = ops.DevicePlan(plan, DEV)
    hp = dict(lr=0.05, momentum=0.9, dampening=0.0, weight_decay=1e-4, nesterov=False)
    grads = [_grad(plan, seed=60 + i).to(DEV) for i in range(3)]
    p0 = torch.randn(plan.length, device=DEV)

    def state():
        return dict(g=torch.zeros(plan.length, device=DEV), r=torch.zeros(plan.length, device=DEV),
                    p=p0.clone(), m=torch.zeros(plan.length, device=DEV),
                    pay=torch.zeros(1, lay.nbytes, dtype=torch.uint8, device=DEV))

    def step(s):
        ops.sign_encode(dp, s["g"], s["pay"][0], lay, resid=s["r"], rot_key=KEY)
        ops.sign_decode_apply(dp, s["pay"], lay, param=s["p"], mom=s["m"], first=False,
                              rot_key=KEY, **hp)

    eager = state()
    for g in grads:
        eager["g"].copy_(g)
        step(eager)
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
    for k in ("p", "m", "r", "pay"):
        assert torch.equal(cap[k], eager[k]), k


def test_bad_operands_rejected():
    """Size, dtype and alignment are checked on the host, before any launch."""
    ops.require()
    plan = _plan([1000, 8192 + 1])
    lay = Layout.build("sign", plan)
    dp = ops.DevicePlan(plan, DEV)
    g = torch.zeros(plan.length, device=DEV)
    pay = torch.zeros(lay.nbytes, dtype=torch.uint8, device=DEV)
    with pytest.raises(ValueError):  # payload too short
        ops.sign_encode(dp, g, pay[:lay.nbytes - 16], lay, rot_key=KEY)
    with pytest.raises(ValueError):  # gradient too short
        ops.sign_encode(dp, g[:100], pay, lay, rot_key=KEY)
    with pytest.raises(TypeError):  # wrong dtypes
        ops.sign_encode(dp, g.double(), pay, lay, rot_key=KEY)
    with pytest.raises(TypeError):
        ops.sign_encode(dp, g, pay, lay, resid=g.to(torch.bfloat16), rot_key=KEY)
    big = torch.zeros(plan.length + 4, device=DEV)
    bigpay = torch.zeros(lay.nbytes + 16, dtype=torch.uint8, device=DEV)
    with pytest.raises(ValueError):  # misaligned views
        ops.sign_encode(dp, big[1:], pay, lay, rot_key=KEY)
    with pytest.raises(ValueError):
        ops.sign_encode(dp, g, bigpay[4:], lay, rot_key=KEY)
    with pytest.raises(ValueError):
        ops.sign_encode(dp, g, pay, lay, resid=big[1:], rot_key=KEY)
    with pytest.raises(ValueError):  # another codec's layout
        ops.sign_encode(dp, g, pay, Layout.build("qsgd", plan, 8), rot_key=KEY)
    recv = pay[None]
    with pytest.raises(ValueError):  # row length is not the layout's
        ops.sign_decode_apply(dp, bigpay[None], lay, grad_out=g, rot_key=KEY)
    with pytest.raises(ValueError):  # nothing to do
        ops.sign_decode_apply(dp, recv, lay, rot_key=KEY)
    with pytest.raises(ValueError):
        ops.sign_decode_apply(dp, recv, lay, param=big[1:], mom=g, rot_key=KEY)
    # the extension's own checks, below the Python wrapper: a missing table, a misaligned operand,
    # sections that do not fit, the slot-addressed form
    C = ops.require()
    ptrs, mask = ops.grad_pointers(dp, g)
    stream = torch.cuda.current_stream().cuda_stream
    def encode(**fields):
        a = dict(resid=0, chunks=dp.chunks.data_ptr(), payload=pay.data_ptr(),
                 payload_bytes=lay.nbytes, num_tensors=plan.num_tensors,
                 num_chunks=plan.num_chunks, scales_off=lay.scales, bits_off=lay.codes,
                 stream=stream, slots=0, slot_end=0, rotate=1, rot_key=KEY)
        a.update(fields)
        C.sign_encode(ops._args(C.SignEncodeArgs, **a), ptrs, mask)

    with pytest.raises(RuntimeError, match="missing table"):
        encode(chunks=0)
    with pytest.raises(RuntimeError, match="misaligned"):
        encode(resid=g.data_ptr() + 4)
    with pytest.raises(RuntimeError, match="do not fit"):
        encode(payload_bytes=lay.nbytes - 16)
    with pytest.raises(RuntimeError, match="slot-addressed"):
        encode(slots=dp.chunks.data_ptr(), slot_end=lay.nbytes)

    def decode(chunks, grad_out):
        C.sign_decode_apply(ops._args(
            C.SignDecodeArgs, recv=pay.data_ptr(), nranks=1, stride=lay.nbytes, chunks=chunks,
            num_chunks=plan.num_chunks, scales_off=lay.scales, bits_off=lay.codes,
            step=C.StepArgs(grad_out=grad_out), stream=stream, slots=0, slot_end=0, rotate=1,
            rot_key=KEY))

    with pytest.raises(RuntimeError, match="missing table"):
        decode(0, g.data_ptr())
    with pytest.raises(RuntimeError, match="misaligned"):
        decode(dp.chunks.data_ptr(), g.data_ptr() + 4)
    torch.cuda.synchronize()
    assert not pay.any() and not g.any()  # nothing ran
