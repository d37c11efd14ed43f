"""The MXFP8 / MXFP4 codec's HIP kernels (ops/csrc/mx_codec.hip) vs the torch oracle, on one MI355X.

Exactness contract: payload bytes (scale bytes, codes and every pad), residuals, decoded sums and
the fused SGD step are bitwise the oracle's; where the oracle holds a NaN the kernels must too.
The boundary tests are the hardware-against-oracle check of the v_cvt_scalef32_pk_* conversions:
every rounding tie of both grids, the saturation band, zeros and fp32 denormals under the smallest,
the largest and the clamped scale bytes.  Every kernel test runs the hardware conversions and the
``soft`` (software) ones.
"""
import pytest
import torch

from ewdml import ops
from ewdml.compress import oracle
from ewdml.compress.plan import BucketPlan, Layout
from ewdml.compress.rng import stream_key

pytestmark = pytest.mark.gpu

DEV = "cuda"

# the sign test's shapes: one-element tensor and a tail shorter than a block | tails of 1..5 | a
# 5-element tail after full chunks, multi-chunk tensors
SHAPES = [[10], [1, 2, 3, 4, 5], [500, 10], [8192 * 3 + 5, 7, 64, 100003]]
BITS = [8, 4]


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


def _same(a, b):
    """Bitwise equality of fp32 tensors, except that a NaN only has to meet a NaN."""
    a, b = a.contiguous(), b.contiguous()
    nan = torch.isnan(b)
    if not torch.equal(torch.isnan(a), nan):
        return False
    return torch.equal(a.view(torch.int32)[~nan], b.view(torch.int32)[~nan])


def _split(plan, g, dtype=torch.float32):
    return [g[o:o + n].clone().to(dtype).to(DEV) for o, n in zip(plan.offsets, plan.numels)]


@pytest.mark.parametrize("ef", [False, True])
@pytest.mark.parametrize("bits", BITS)
@pytest.mark.parametrize("numels", SHAPES)
def test_encode_matches_oracle(numels, bits, ef):
    ops.require()
    plan = _plan(numels)
    lay = Layout.build("mx", plan, bits)
    dp = ops.DevicePlan(plan, DEV)
    pay = torch.full((lay.nbytes,), 0xFF, dtype=torch.uint8, device=DEV)  # every byte is rewritten
    soft = torch.full((lay.nbytes,), 0xFF, dtype=torch.uint8, device=DEV)
    r_ref = _grad(plan, seed=50) * 0.3 if ef else None
    r_dev = r_ref.to(DEV) if ef else None
    for it in range(2):
        g = _grad(plan, seed=len(numels) + it)
        r_soft = r_dev.clone() if ef else None
        ref = oracle.encode_mx(g.clone(), plan, lay, r_ref)
        ops.mx_encode(dp, g.to(DEV), pay, lay, resid=r_dev)
        ops.mx_encode(dp, g.to(DEV), soft, lay, resid=r_soft, soft=True)
        for name, got, res in (("hardware", pay.cpu(), r_dev), ("soft", soft.cpu(), r_soft)):
            assert torch.equal(got, ref), \
                f"{name} encode {it}: payload differs at {(got != ref).nonzero()[:10].flatten()}"
            if ef:
                assert _same(res.cpu(), r_ref), f"{name} encode {it}: residual"


@pytest.mark.parametrize("bits", BITS)
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_encode_from_per_tensor_pointers(dtype, bits):
    """Autograd's own per-tensor gradients (fp32 or bf16, read through the pointer table), with
    the error feedback staged in the fp32 residual; the gradients are not modified."""
    ops.require()
    plan = _plan([8192 + 7, 64, 30000, 5], bucket_offset=256)
    lay = Layout.build("mx", plan, bits)
    g = _grad(plan, seed=3)
    for o, n in zip(plan.offsets, plan.numels):  # the flat reference holds the same values
        g[o:o + n] = g[o:o + n].to(dtype).float()
    dp = ops.DevicePlan(plan, DEV)
    pay = torch.zeros(lay.nbytes, dtype=torch.uint8, device=DEV)
    grads = _split(plan, g, dtype)
    before = [t.clone() for t in grads]
    ops.mx_encode(dp, grads, pay, lay)
    assert torch.equal(pay.cpu(), oracle.encode_mx(g.clone(), plan, lay))
    r_ref = _grad(plan, seed=8) * 0.05
    r_dev = r_ref.to(DEV)
    ref = oracle.encode_mx(g.clone(), plan, lay, r_ref)
    ops.mx_encode(dp, grads, pay, lay, resid=r_dev)
    assert torch.equal(pay.cpu(), ref)
    assert _same(r_dev.cpu(), r_ref)
    for a, b in zip(grads, before):
        assert torch.equal(a, b)


# ---- the boundary tensor -------------------------------------------------------------------------
EMS = [0, 1, 8, 9, 127, 253, 254]  # exponent field of the block's largest element
DENORMALS = [0x00000001, 0x00000003, 0x00400000, 0x005FFFFF]


def _grid(bits):
    """The non-negative values of the element grid, ascending (fp64)."""
    n = 1 << (bits - 1)
    codes = torch.arange(n, dtype=torch.uint8).reshape(1, -1)
    pad = torch.zeros(1, 32 * ((n + 31) // 32) - n, dtype=torch.uint8)
    v = oracle.mx_dequantize(torch.cat([codes, pad], 1).reshape(-1, 32),
                             torch.full(((n + 31) // 32,), 127, dtype=torch.int64), bits)
    v = v.flatten()[:n].double()
    return v[~torch.isnan(v)]  # E4M3's 0x7F is NaN


def _ulp_neighbours(x):
    b = x.view(torch.int32)
    return torch.cat([(b - 1).view(torch.float32), x, (b + 1).view(torch.float32)])


def _boundary(bits):
    """fp32 [B, 32]: for every em of EMS, blocks whose largest element has that exponent field
    and which hold, scaled by the block's X = 2^(s - 127): every midpoint between neighbouring
    grid values and its two fp32 neighbours, the saturation band, +/-0.0 and fp32 denormals, all of
    both signs; then one block holding an inf and one holding a NaN."""
    emax, top = oracle.MX_FORMATS[bits][4], oracle.MX_FORMATS[bits][3]
    v = _grid(bits)
    mids = (v[:-1] + v[1:]) / 2
    lim = 2.0 ** (emax + 1)  # the band (top, lim) saturates: the scale rule takes the floor
    band = torch.tensor([top * (1 + 2.0 ** -23), top * 1.002, (top + lim) / 2 * (1 - 2.0 ** -24),
                         (top + lim) / 2, (top + 3 * lim) / 4, lim * (1 - 2.0 ** -24),
                         top, top * (1 - 2.0 ** -24)], dtype=torch.float64)
    blocks = []
    for em in EMS:
        s = max(em - emax, 0)
        X, limit = 2.0 ** (s - 127), 2.0 ** (em - 126)
        vals = _ulp_neighbours((mids * X).float())
        vals = torch.cat([vals, (band * X).float()])
        vals = vals[vals.double().abs() < limit]
        vals = torch.stack([vals, -vals], 1).flatten()
        anchor = torch.tensor([0x00600000 if em == 0 else (em << 23) | 0x00400000],
                              dtype=torch.int32).view(torch.float32)  # 1.5 * 2^(em - 127)
        per = 32 - 5
        for i in range(0, vals.numel(), per):
            den = torch.tensor([DENORMALS[(i // per) % 4]], dtype=torch.int32).view(torch.float32)
            fixed = torch.cat([anchor if (i // per) % 2 else -anchor, torch.tensor([0.0, -0.0]),
                               den, -den])
            blk = torch.cat([vals[i:i + per], fixed])
            blk = torch.cat([blk, torch.zeros(32 - blk.numel())])
            blocks.append(blk[torch.randperm(32, generator=torch.Generator().manual_seed(i))])
    if len(blocks) % 2:  # the bucket is a whole number of 64-element units
        blocks.append(torch.zeros(32))
    for bad in (float("inf"), float("nan")):
        blk = torch.linspace(-3, 3, 32)
        blk[7] = bad
        blocks.append(blk)
    return torch.stack(blocks)


def _report(x, got, ref, bits, what):
    """The first positions where two code / value arrays differ, for the assertion message."""
    bad = (got != ref).nonzero().flatten()
    lines = [f"{what}: {bad.numel()} of {ref.numel()} differ"]
    for i in bad[:24].tolist():
        lines.append(f"  [{i}] input {int(x.view(torch.int32)[i]) & 0xFFFFFFFF:#010x} "
                     f"({float(x[i])!r}) got {int(got[i]):#x} want {int(ref[i]):#x}")
    return "\n".join(lines)


@pytest.mark.parametrize("soft", [False, True], ids=["hardware", "soft"])
@pytest.mark.parametrize("bits", BITS)
def test_boundary_tensor(bits, soft):
    ops.require()
    blocks = _boundary(bits)
    g = blocks.flatten()
    plan = _plan([g.numel()])
    assert plan.length == g.numel()
    lay = Layout.build("mx", plan, bits)
    dp = ops.DevicePlan(plan, DEV)
    r_ref = torch.zeros(plan.length)
    r_dev = r_ref.to(DEV)
    ref = oracle.encode_mx(g.clone(), plan, lay, r_ref)
    pay = torch.full((lay.nbytes,), 0xFF, dtype=torch.uint8, device=DEV)
    ops.mx_encode(dp, g.to(DEV), pay, lay, resid=r_dev, soft=soft)
    got = pay.cpu()
    nb = g.numel() // 32
    assert torch.equal(got[:nb], ref[:nb]), _report(
        blocks.abs().max(1).values, got[:nb], ref[:nb], bits, "scale bytes")
    gc, rc = got[lay.codes:], ref[lay.codes:]
    if bits == 4:
        gc, rc = (torch.stack([c & 0xF, c >> 4], 1).flatten() for c in (gc, rc))
    assert torch.equal(gc[:g.numel()], rc[:g.numel()]), _report(
        g, gc[:g.numel()], rc[:g.numel()], bits, "codes")
    assert torch.equal(got, ref)
    rd = r_dev.cpu()
    assert torch.isnan(r_ref[-64:]).all() and torch.isnan(rd[-64:]).all()  # the inf and NaN blocks
    assert _same(rd, r_ref), _report(g, rd.view(torch.int32), r_ref.view(torch.int32), bits,
                                     "residual bits")
    # and back: the receive side decodes what was sent to the oracle's values
    out = torch.zeros(plan.length, device=DEV)
    ops.mx_decode_apply(dp, pay[None], lay, grad_out=out, soft=soft)
    want = oracle.decode_sum(ref[None], plan, lay, 0, 1.0)
    assert _same(out.cpu(), want), _report(g, out.cpu().view(torch.int32),
                                           want.view(torch.int32), bits, "decoded bits")


@pytest.mark.parametrize("soft", [False, True], ids=["hardware", "soft"])
@pytest.mark.parametrize("bits", BITS)
def test_decode_every_code_under_every_scale(bits, soft):
    """A hand-made payload: every code of the format under the smallest scale bytes (decoded
    values are fp32 denormals there), middle ones, the largest an encode writes and 0xFF."""
    ops.require()
    top_s = 254 - oracle.MX_FORMATS[bits][4]
    scales = [0, 1, 2, 9, 10, 118, 126, 127, 128, 200, top_s - 1, top_s, 255]
    n = 1 << bits
    codes = torch.arange(n, dtype=torch.uint8)
    if bits == 8:  # the two NaN codes are never sent
        codes[0x7F], codes[0xFF] = 0x7E, 0xFE
    per = max(n, 64)
    plan = _plan([per * len(scales)])
    lay = Layout.build("mx", plan, bits)
    pay = torch.zeros(lay.nbytes, dtype=torch.uint8)
    body = codes.repeat(per // n).repeat(len(scales))
    pay[:plan.length // 32] = torch.tensor(scales, dtype=torch.uint8).repeat_interleave(per // 32)
    if bits == 4:
        body = body[0::2] | (body[1::2] << 4)
    pay[lay.codes:lay.codes + body.numel()] = body
    recv = torch.stack([pay, pay])
    want = oracle.decode_sum(recv[:1], plan, lay, 0, 1.0)
    assert torch.isfinite(want[:-per]).all() and torch.isnan(want[-per:]).all()
    dp = ops.DevicePlan(plan, DEV)
    out = torch.zeros(plan.length, device=DEV)
    ops.mx_decode_apply(dp, recv[:1].to(DEV), lay, grad_out=out, soft=soft)
    assert _same(out.cpu(), want), _report(want, out.cpu().view(torch.int32),
                                           want.view(torch.int32), bits, "decoded bits")
    ops.mx_decode_apply(dp, recv.to(DEV), lay, grad_out=out, grad_scale=0.5, soft=soft)
    assert _same(out.cpu(), oracle.decode_sum(recv, plan, lay, 0, 0.5))


# ---- the receive side -----------------------------------------------------------------------------
ROWS_PLAN = [9000, 64, 33, 8192 + 3, 1]


def _payloads(plan, lay, N, seed=100):
    # very different magnitudes per rank: the rank order of the fp32 sum matters
    return torch.stack([oracle.encode_mx(_grad(plan, seed=seed + r) * (3.0 ** r), plan, lay)
                        for r in range(N)])


_DECODED = {}


def _rows(bits, N):
    """(plan, layout, received rows, their decoded mean), computed once per case and only read."""
    if (bits, N) not in _DECODED:
        plan = _plan(ROWS_PLAN, bucket_offset=128)
        lay = Layout.build("mx", plan, bits)
        recv = _payloads(plan, lay, N)
        _DECODED[bits, N] = (plan, lay, recv, oracle.decode_sum(recv, plan, lay, 0, 1.0 / N))
    return _DECODED[bits, N]


# lr = 2^-4 and dampening = 0: lr * d and (1 - dampening) * d are exact, so the reference does not
# depend on whether torch's CPU ``add_(x, alpha=)`` contracts its multiply-add (the kernels never
# do); every other step of oracle.sgd_apply is a separately rounded operation
PLAIN = dict(lr=0.0625, momentum=0.0, dampening=0.0, weight_decay=0.0, nesterov=False)
NESTEROV = dict(lr=0.0625, momentum=0.9, dampening=0.0, weight_decay=5e-4, nesterov=True)


@pytest.mark.parametrize("hp,first", [(PLAIN, False), (NESTEROV, True), (NESTEROV, False)],
                         ids=["plain", "nesterov-first", "nesterov-later"])
@pytest.mark.parametrize("N", [1, 2, 3, 8])
@pytest.mark.parametrize("bits", BITS)
def test_decode_apply_rows(bits, N, hp, first):
    ops.require()
    plan, lay, recv, g = _rows(bits, N)
    with_mom = hp["momentum"] != 0
    gen = torch.Generator().manual_seed(11)
    p0 = torch.randn(plan.length, generator=gen)
    m0 = torch.randn(plan.length, generator=gen)
    p, m = p0.clone(), m0.clone()
    for off, n in zip(plan.offsets, plan.numels):
        oracle.sgd_apply(p[off:off + n], m[off:off + n] if with_mom else None, g[off:off + n],
                         first=first, **hp)
    dp = ops.DevicePlan(plan, DEV)
    pd, md = p0.to(DEV), m0.to(DEV)
    go = torch.full((plan.length,), float("nan"), device=DEV)
    sh = torch.zeros(plan.length, dtype=torch.bfloat16, device=DEV)
    seed, step, rank = 5, 41, 3
    ks = torch.tensor([step, 0], dtype=torch.int32, device=DEV)
    lr_t = torch.tensor([hp["lr"]], device=DEV)  # the device scalar wins over the host value
    ops.mx_decode_apply(dp, recv.to(DEV), lay, param=pd, mom=md if with_mom else None,
                        grad_out=go, grad_scale=1.0 / N, first=first, shadow=sh, key_state=ks,
                        key_seed=seed, key_rank=rank, lr_tensor=lr_t, **dict(hp, lr=999.0))
    assert _same(pd.cpu(), p)
    assert _same(md.cpu(), m)  # untouched when there is no momentum
    got = go.cpu()
    own = torch.zeros(plan.length, dtype=torch.bool)
    for off, n in zip(plan.offsets, plan.numels):
        own[off:off + n] = True
        assert torch.equal(sh[off:off + n].cpu(), p[off:off + n].to(torch.bfloat16))
    assert _same(got[own], g[own])
    assert torch.isnan(got[~own]).all()  # nothing is written between the tensors
    assert [int(v) & 0xFFFFFFFF for v in ks.cpu()] == [step + 1, stream_key(seed, step + 1, rank)]


@pytest.mark.parametrize("bits", BITS)
def test_encode_decode_graph_capture(bits):
    """Encode + decode-apply captured on one stream and replayed with fresh gradients copied into
    the static buffers: bitwise the eager run (no scratch, no memset, no host state)."""
    ops.require()
    plan = _plan([8192 * 2 + 5, 700, 3])
    lay = Layout.build("mx", plan, bits)
    dp = ops.DevicePlan(plan, DEV)
    hp = dict(lr=0.05, momentum=0.9, dampening=0.0, weight_decay=1e-4, nesterov=False)
    grads = [_grad(plan, seed=60 + i).to(DEV) for i in range(3)]
    p0 = torch.randn(plan.length, device=DEV)

    def state():
        return dict(g=torch.zeros(plan.length, device=DEV), r=torch.zeros(plan.length, device=DEV),
                    p=p0.clone(), m=torch.zeros(plan.length, device=DEV),
                    pay=torch.zeros(1, lay.nbytes, dtype=torch.uint8, device=DEV))

    def step(s):
        ops.mx_encode(dp, s["g"], s["pay"][0], lay, resid=s["r"])
        ops.mx_decode_apply(dp, s["pay"], lay, param=s["p"], mom=s["m"], first=False, **hp)

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
    assert eager["r"].abs().max() > 0


def test_bad_operands_rejected():
    """Size, dtype, alignment and the layout are checked on the host, before any launch."""
    ops.require()
    plan = _plan([1000, 8192 + 1])
    lay = Layout.build("mx", plan, 8)
    dp = ops.DevicePlan(plan, DEV)
    g = torch.zeros(plan.length, device=DEV)
    pay = torch.zeros(lay.nbytes, dtype=torch.uint8, device=DEV)
    bigpay = torch.zeros(lay.nbytes + 16, dtype=torch.uint8, device=DEV)
    big = torch.zeros(plan.length + 4, device=DEV)
    with pytest.raises(ValueError):  # payload too short
        ops.mx_encode(dp, g, pay[:lay.nbytes - 16], lay)
    with pytest.raises(ValueError):  # gradient too short
        ops.mx_encode(dp, g[:100], pay, lay)
    with pytest.raises(TypeError):
        ops.mx_encode(dp, g.double(), pay, lay)
    with pytest.raises(TypeError):
        ops.mx_encode(dp, g, pay, lay, resid=g.to(torch.bfloat16))
    with pytest.raises(ValueError):  # misaligned views
        ops.mx_encode(dp, g, bigpay[4:], lay)
    with pytest.raises(ValueError):
        ops.mx_encode(dp, g, pay, lay, resid=big[1:])
    with pytest.raises(ValueError):  # another codec's layout, another plan's layout
        ops.mx_encode(dp, g, pay, Layout.build("sign", plan))
    with pytest.raises(ValueError):
        ops.mx_encode(dp, g, pay, Layout.build("mx", _plan([1000, 8192 + 1, 64]), 8))
    with pytest.raises(ValueError):  # row length is not the layout's
        ops.mx_decode_apply(dp, bigpay[None], lay, grad_out=g)
    with pytest.raises(ValueError):  # nothing to do
        ops.mx_decode_apply(dp, pay[None], lay)
    with pytest.raises(ValueError):
        ops.mx_decode_apply(dp, pay[None], lay, param=g, mom=None, lr=0.0625, momentum=0.9)
    torch.cuda.synchronize()
    assert not pay.any() and not g.any()  # nothing ran
