"""Dense QSGD's HIP kernels (ops/csrc/qsgd_codec.hip: k_qsgd_stats, k_qsgd_scale, k_qsgd_quant,
k_qsgd_decode_apply) vs the torch oracle and float64, on one MI355X.

Exactness contract: under the max norm the payload (scales, int8 / int4 codes, pads), the residual,
the decoded sum, the fused SGD step and the key advance are bitwise the oracle's.  Under the L2
norm one quantity has a tolerance, the scale, whose fp32 sum of squares runs in the kernel's own
order: it is held to the bound derived at ``_scale_bound``, and every code and residual is then
bitwise the oracle's rounding under the scale the device wrote.

The payloads are zero-filled before an encode, as the exchange allocates them: the kernels write
the scales and, per tensor, the codes of its elements rounded up to 4; the rest of a tensor's 16
code slots and the sections' alignment pads are never written (``_owned``)."""
import math

import pytest
import torch

from ewdml import ops
from ewdml.compress import oracle
from ewdml.compress.plan import Layout
from ewdml.compress.rng import stream_key, uniform
from tests import qsgd_sim as sim

pytestmark = pytest.mark.gpu

DEV = "cuda"
BITS = [(8, 127), (4, 7)]
BIT_IDS = ["int8", "int4"]
EFS = [False, True]
EF_IDS = ["plain", "ef"]
# every tail length mod 4, odd code counts for the nibble pairs, the chunk boundaries
EDGE = [1, 2, 3, 4, 5, 63, 64, 8191, 8192, 8193, 8192 * 3 + 5]
# the one plan with a tensor of more than EW_BLOCK = 256 chunks (288: a VGG-11 conv weight)
MANY = [2359296, 7]
MIX = [8192 + 13, 10, 5000]
PLANS = {"edge": EDGE, "mix": MIX, "many": MANY}
SEED = 7
KEY = stream_key(SEED, 11, 2)
GUARD, SENT = 64, 0xA5  # sentinel bytes either side of a payload
G_GAP, R_GAP = 1.0e4, -1.0e4  # between the tensors: never read (it would swamp a scale) or written


def _bits(t):
    return t.contiguous().view(torch.int32)


_PLANS = {}


def _plan(name):
    """The plan of a name of PLANS or of a tuple of tensor sizes, at a non-zero bucket offset."""
    if name not in _PLANS:
        _PLANS[name] = sim.make_plan(PLANS[name] if isinstance(name, str) else name)
    return _PLANS[name]


def _ranges(plan):
    return list(zip(plan.offsets, plan.numels))


def _own(plan):
    own = torch.zeros(plan.length, dtype=torch.bool)
    for off, n in _ranges(plan):
        own[off:off + n] = True
    return own


_BUCKETS = {}


def _bucket(name, seed, gap=G_GAP):
    """A bucket of random tensors (only read: clone before changing it), ``gap`` between them."""
    if (name, seed, gap) not in _BUCKETS:
        _BUCKETS[(name, seed, gap)] = sim.bucket(_plan(name), seed, gap)
    return _BUCKETS[(name, seed, gap)]


def _resid(name):
    """A starting residual of the gradient's magnitude."""
    return _bucket(name, 91, R_GAP)


def _scales(pay, plan, lay):
    return oracle._section(pay, lay.scales, plan.num_tensors, torch.float32)


def _codes(pay, plan, lay):
    """int32 codes of every slot of the codes section, pads included."""
    if lay.bits == 8:
        return oracle._section(pay, lay.codes, plan.total_codes, torch.int8).to(torch.int32)
    return oracle._unpack4(pay[lay.codes:lay.codes + plan.total_codes // 2], plan.total_codes)


def _code_bytes(pay, plan, lay, t):
    """The bytes of tensor t's 16-aligned slots in the codes section."""
    d0, n = plan.tensor_code0[t], (plan.numels[t] + 15) // 16 * 16
    per = 1 if lay.bits == 8 else 2
    return pay[lay.codes + d0 // per:lay.codes + (d0 + n) // per]


def _owned(plan, lay):
    """The payload bytes an encode writes: the scales and, per tensor, the codes of its elements
    rounded up to 4 (one 32-bit word of int8 codes or one 16-bit word of nibbles per thread)."""
    m = torch.zeros(lay.nbytes, dtype=torch.bool)
    m[lay.scales:lay.scales + 4 * plan.num_tensors] = True
    per = 1 if lay.bits == 8 else 2
    for d0, n in zip(plan.tensor_code0, plan.numels):
        m[lay.codes + d0 // per:lay.codes + (d0 + (n + 3) // 4 * 4) // per] = True
    return m


def _enc(dp, lay, levels, norm, g, key=KEY, r=None, fill=0, **kw):
    """One device encode of the CPU bucket ``g`` (residual ``r``) into a payload pre-filled with
    ``fill`` between sentinel guards.  Returns the payload and the residual, on the CPU; the
    guards, the gradient and the residual's gaps must come back untouched."""
    plan = dp.plan
    buf = torch.full((lay.nbytes + 2 * GUARD,), SENT, dtype=torch.uint8, device=DEV)
    pay = buf[GUARD:GUARD + lay.nbytes]
    pay.fill_(fill)
    gd = g.to(DEV)
    rd = None if r is None else r.to(DEV)
    ops.qsgd_encode(dp, gd, pay, lay, levels, norm, key, resid=rd, **kw)
    out = buf.cpu()
    assert bool((out[:GUARD] == SENT).all()) and bool((out[-GUARD:] == SENT).all()), \
        "wrote outside the payload"
    assert torch.equal(_bits(gd.cpu()), _bits(g)), "the gradient was modified"
    if r is not None:
        rd = rd.cpu()
        assert bool((rd[~_own(plan)] == R_GAP).all()), "wrote between the tensors of the residual"
    return out[GUARD:GUARD + lay.nbytes].clone(), rd


def _dec(dp, lay, levels, rows, **kw):
    """The device decode of the CPU payload rows [N, nbytes] into a NaN-prefilled grad_out."""
    go = torch.full((dp.plan.length,), float("nan"), device=DEV)
    ops.qsgd_decode_apply(dp, rows.to(DEV), lay, levels, grad_out=go, **kw)
    return go.cpu()


# ---- 1. max norm: bitwise the oracle ------------------------------------------------------------
@pytest.mark.parametrize("ef", EFS, ids=EF_IDS)
@pytest.mark.parametrize("bits,levels", BITS, ids=BIT_IDS)
@pytest.mark.parametrize("name", ["edge", "mix"])
def test_encode_max_norm_is_the_oracle(name, bits, levels, ef):
    ops.require()
    _check_max_encode(name, bits, levels, ef)


def test_encode_max_norm_many_chunks():
    """The max-norm encode of the plan whose tensor has more than 256 chunks."""
    ops.require()
    _check_max_encode("many", 8, 127, False)


def _check_max_encode(name, bits, levels, ef):
    plan = _plan(name)
    lay = Layout.build("qsgd", plan, bits)
    dp = ops.DevicePlan(plan, DEV)
    g = _bucket(name, 1)
    r_ref = _resid(name).clone() if ef else None
    ref = oracle.encode_qsgd(g.clone(), plan, lay, levels, "max", KEY, r_ref)
    got, r_dev = _enc(dp, lay, levels, "max", g, r=_resid(name) if ef else None)
    sg, sr = _scales(got, plan, lay), _scales(ref, plan, lay)
    assert torch.equal(_bits(sg), _bits(sr)), f"scales {sg} vs {sr}"
    assert torch.equal(got, ref), f"payload differs at {(got != ref).nonzero()[:10].flatten()}"
    assert int(_codes(ref, plan, lay).abs().max()) == levels  # the largest element saturates
    if ef:
        for off, n in _ranges(plan):
            assert torch.equal(_bits(r_dev[off:off + n]), _bits(r_ref[off:off + n])), off
        assert float(r_dev[_own(plan)].abs().max()) > 0
    # every byte the kernels own is written, zero codes included, and no other: the same encode
    # over a sentinel-filled payload
    own = _owned(plan, lay)
    got2, _ = _enc(dp, lay, levels, "max", g, r=_resid(name) if ef else None, fill=SENT)
    assert torch.equal(got2[own], ref[own])
    assert bool((got2[~own] == SENT).all())


@pytest.mark.parametrize("bits,levels", BITS, ids=BIT_IDS)
def test_bernoulli_tie_rounds_down(bits, levels):
    """The rounding goes up when ``u < frac``, strictly.  A tie has probability 2^-24 per element,
    so random data never meets one: here every element is its own variate (the scale is
    ``levels``, so ``levels / scale`` is 1 and an element's level is its magnitude), and next to
    it the same elements one step of 2^-24 above the tie."""
    ops.require()
    n = 8192 + 5
    plan = _plan((n, 64))
    lay = Layout.build("qsgd", plan, bits)
    dp = ops.DevicePlan(plan, DEV)
    g = _bucket((n, 64), 3).clone()
    off = plan.offsets[0]
    u = uniform(plan.bucket_offset + off + torch.arange(n), KEY)
    sign = torch.where(torch.arange(n) % 3 == 0, -1.0, 1.0)
    for bump, want in ((0.0, 0), (2.0 ** -24, 1)):
        x = (u + bump) * sign
        x[n - 1] = float(levels)
        g[off:off + n] = x
        ref = oracle.encode_qsgd(g.clone(), plan, lay, levels, "max", KEY)
        q = _codes(ref, plan, lay)[plan.tensor_code0[0]:plan.tensor_code0[0] + n]
        assert float(_scales(ref, plan, lay)[0]) == levels
        assert torch.equal(q[:n - 1], (want * sign[:n - 1]).to(torch.int32))  # what is under test
        got, _ = _enc(dp, lay, levels, "max", g)
        assert torch.equal(got, ref), f"bump {bump}"


# ---- 2, 3. L2 norm: the scale against float64, everything else exact under that scale -----------
U = 2.0 ** -24  # unit roundoff of fp32


def _scale_bound(plan):
    """(additions, bound): the relative error allowed to the device's L2 scale.

    The additions a square meets on the longest path to the tensor's total, in the kernels' order:
      32  k_qsgd_stats: a thread's serial ``sq = sq + x * x`` over its 4 elements of each of the
          8192 / (4 * 256) = 8 slabs of a chunk
       6  ew_wave_sum: log2(64) shuffle steps
       4  ew_block_sum: ``s += wsf[i]`` over the 4 wave partials
       m  k_qsgd_scale: a thread's strided ``sq = sq + chunk_sq[j]``, m = ceil(nchunks / 256)
       6  ew_wave_sum again
       4  ew_block_sum again
    = 52 + m: 53 for up to 256 chunks, 54 for the 288 of MANY.  Every term is a non-negative fp32
    product x * x (one more rounding), so the computed sum is within a factor (1 + U)^(adds + 1)
    of the exact one; the square root halves that, and sqrtf rounds once more."""
    m = max(math.ceil(nc / 256) for nc in plan.tensor_nchunks)
    adds = 32 + 6 + 4 + m + 6 + 4
    return adds, math.sqrt((1 + U) ** (adds + 1)) * (1 + U) - 1


_L2 = {}


def _l2_case(name, bits, levels, ef):
    """(plan, layout, what is quantised: g or the fp32 g + r, payload, residual) of one L2 encode
    on the device, computed once per case and only read."""
    k = (name, bits, ef)
    if k not in _L2:
        plan = _plan(name)
        lay = Layout.build("qsgd", plan, bits)
        g = _bucket(name, 2)
        e = g + _resid(name) if ef else g
        pay, r = _enc(ops.DevicePlan(plan, DEV), lay, levels, "l2", g,
                      r=_resid(name) if ef else None)
        _L2[k] = (plan, lay, e, pay, r)
    return _L2[k]


@pytest.mark.parametrize("ef", EFS, ids=EF_IDS)
@pytest.mark.parametrize("name", ["edge", "mix", "many"])
def test_l2_scale_against_float64(name, ef):
    """Would fail if k_qsgd_scale's strided loop dropped or double-counted a chunk (a tensor of one
    chunk would come out 0 or sqrt(2) times too large)."""
    ops.require()
    plan, lay, e, pay, _ = _l2_case(name, 8, 127, ef)
    adds, bound = _scale_bound(plan)
    assert adds == (54 if name == "many" else 53) and bound < 1e-5
    s = _scales(pay, plan, lay).double()
    worst = 0.0
    for t, (off, n) in enumerate(_ranges(plan)):
        ref = float(e[off:off + n].double().norm())
        worst = max(worst, abs(float(s[t]) - ref) / ref)
    print(f"\nqsgd-l2-scale plan={name} ef={int(ef)} adds={adds} bound={bound:.4e} "
          f"worst={worst:.4e} ratio={worst / bound:.4f}")
    assert worst <= bound


L2_CASES = [(n, b, lv) for n in ("edge", "mix") for b, lv in BITS] + [("many", 8, 127)]


@pytest.mark.parametrize("ef", EFS, ids=EF_IDS)
@pytest.mark.parametrize("name,bits,levels", L2_CASES, ids=[f"{n}-int{b}" for n, b, _ in L2_CASES])
def test_l2_codes_exact_under_the_device_scale(name, bits, levels, ef):
    ops.require()
    plan, lay, e, pay, r = _l2_case(name, bits, levels, ef)
    s = _scales(pay, plan, lay)
    codes = _codes(pay, plan, lay)
    for t, (off, n) in enumerate(_ranges(plan)):
        x, scale, d0 = e[off:off + n], float(s[t]), plan.tensor_code0[t]
        gidx = plan.bucket_offset + off + torch.arange(n)
        q = oracle.quantize(x, scale, levels, gidx, KEY)
        assert torch.equal(codes[d0:d0 + n], q), f"tensor {t}"
        assert not codes[d0 + n:d0 + (n + 15) // 16 * 16].any(), f"pad codes of tensor {t}"
        if ef:
            want = x - q.to(torch.float32) * oracle.dequant_step(levels, scale)
            assert torch.equal(_bits(r[off:off + n]), _bits(want)), f"residual of tensor {t}"
    assert 0 < int(codes.abs().max()) <= levels


# ---- 4. a second encode on the same DevicePlan --------------------------------------------------
@pytest.mark.parametrize("bits,levels", BITS, ids=BIT_IDS)
@pytest.mark.parametrize("norm", ["max", "l2"])
def test_smaller_gradient_after_a_larger_one(norm, bits, levels):
    """The max key is an atomicMax into scratch: what the first encode left there must not reach
    the second one's scale."""
    ops.require()
    plan = _plan("mix")
    lay = Layout.build("qsgd", plan, bits)
    dp = ops.DevicePlan(plan, DEV)
    g = _bucket("mix", 4)
    small = g * 2.0 ** -6
    first, _ = _enc(dp, lay, levels, norm, g)
    second, _ = _enc(dp, lay, levels, norm, small)
    s1, s2 = _scales(first, plan, lay), _scales(second, plan, lay)
    assert torch.equal(_bits(s2), _bits(s1 * 2.0 ** -6)), f"{s2} vs {s1} / 64"
    assert torch.equal(second[lay.codes:], first[lay.codes:])
    if norm == "max":
        assert torch.equal(second, oracle.encode_qsgd(small.clone(), plan, lay, levels, norm, KEY))
    again, _ = _enc(dp, lay, levels, norm, g)
    assert torch.equal(again, first)


# ---- 5. the key read from device memory ---------------------------------------------------------
@pytest.mark.parametrize("ef", EFS, ids=EF_IDS)
@pytest.mark.parametrize("bits,levels", BITS, ids=BIT_IDS)
def test_key_from_device_memory(bits, levels, ef):
    ops.require()
    plan = _plan("edge")
    lay = Layout.build("qsgd", plan, bits)
    dp = ops.DevicePlan(plan, DEV)
    g = _bucket("edge", 5)
    state = [12, KEY - (1 << 32) if KEY >= 1 << 31 else KEY]
    ks = torch.tensor(state, dtype=torch.int32, device=DEV)
    out = [_enc(dp, lay, levels, "max", g, r=_resid("edge") if ef else None, **kw)
           # the device key wins over the host's
           for kw in (dict(key=KEY), dict(key=0x5A5A5A5A, key_tensor=ks[1:2]))]
    assert ks.tolist() == state
    assert torch.equal(out[0][0], out[1][0])
    r_ref = _resid("edge").clone() if ef else None
    ref = oracle.encode_qsgd(g.clone(), plan, lay, levels, "max", KEY, r_ref)
    assert torch.equal(out[1][0], ref)
    wrong = oracle.encode_qsgd(g.clone(), plan, lay, levels, "max", 0x5A5A5A5A)
    assert not torch.equal(out[1][0], wrong)
    if ef:
        assert torch.equal(_bits(out[0][1]), _bits(out[1][1]))


# ---- 6. a power of two in, the same power of two out --------------------------------------------
# At +-70 the fp32 squares of the L2 norm overflow or underflow, as the reference's fp32
# tensor.norm() also does (the supported range is stated at the top of qsgd_codec.hip): that is not
# tested.  The max norm is a bit pattern and has no such limit.
POW2 = [("max", e) for e in (-70, -40, 40, 70)] + [("l2", e) for e in (-40, 40)]
_BASE = {}


@pytest.mark.parametrize("bits,levels", BITS, ids=BIT_IDS)
@pytest.mark.parametrize("norm,e", POW2, ids=[f"{n}{e:+d}" for n, e in POW2])
def test_power_of_two_scale_invariance(norm, e, bits, levels):
    """Every operation from the gradient to the codes scales exactly by 2^e (sqrtf of a sum times
    2^(2e) included): the codes are bitwise those of the unscaled gradient, the scale 2^e times."""
    ops.require()
    plan = _plan("mix")
    lay = Layout.build("qsgd", plan, bits)
    g = _bucket("mix", 6)
    if (norm, bits) not in _BASE:
        _BASE[(norm, bits)] = _enc(ops.DevicePlan(plan, DEV), lay, levels, norm, g)[0]
    base = _BASE[(norm, bits)]
    f = 2.0 ** e
    # what the norm is taken of stays a normal number, so the scaling is exact
    x = g.double()[_own(plan)].abs() * f
    lo, hi = (float(x.min()), float(x.max())) if norm == "max" else (float(x.min()) ** 2,
                                                                     float((x * x).sum()))
    assert lo > 2.0 ** -126 and hi < 2.0 ** 120
    got, _ = _enc(ops.DevicePlan(plan, DEV), lay, levels, norm, g * f)
    assert torch.equal(got[lay.codes:], base[lay.codes:])
    s = _scales(base, plan, lay)
    assert torch.equal(_bits(_scales(got, plan, lay)), _bits(s * f)) and bool((s * f > 0).all())


# ---- 7. zero and non-finite tensors -------------------------------------------------------------
@pytest.mark.parametrize("ef", EFS, ids=EF_IDS)
@pytest.mark.parametrize("bits,levels", BITS, ids=BIT_IDS)
@pytest.mark.parametrize("norm", ["max", "l2"])
def test_zero_and_non_finite_tensors(norm, bits, levels, ef):
    ops.require()
    plan = _plan("mix")
    lay = Layout.build("qsgd", plan, bits)
    dp = ops.DevicePlan(plan, DEV)
    off1, n1 = plan.offsets[1], plan.numels[1]
    g0 = _bucket("mix", 8)

    def run(g, r):
        pay, res = _enc(dp, lay, levels, norm, g, r=r if ef else None)
        return pay, res, _dec(dp, lay, levels, pay[None])

    def others_unaffected(got, what):
        for t in (0, 2):
            off, n = plan.offsets[t], plan.numels[t]
            assert torch.equal(_bits(_scales(got[0], plan, lay)[t:t + 1]),
                               _bits(_scales(base[0], plan, lay)[t:t + 1])), (what, t)
            assert torch.equal(_code_bytes(got[0], plan, lay, t),
                               _code_bytes(base[0], plan, lay, t)), (what, t)
            assert torch.equal(_bits(got[2][off:off + n]), _bits(base[2][off:off + n])), (what, t)
            assert bool(torch.isfinite(got[2][off:off + n]).all()) and got[2][off:off + n].any()
            if ef:
                assert torch.equal(_bits(got[1][off:off + n]), _bits(base[1][off:off + n]))

    base = run(g0, _resid("mix"))
    # tensor 1 all zeros (under EF: g + r is +0.0 everywhere, from r = -g)
    g = g0.clone()
    r = _resid("mix").clone()
    if ef:
        r[off1:off1 + n1] = -g[off1:off1 + n1]
    else:
        g[off1:off1 + n1] = 0.0
    zero = run(g, r)
    others_unaffected(zero, "zero")
    assert int(_bits(_scales(zero[0], plan, lay))[1]) == 0  # +0.0
    assert not _code_bytes(zero[0], plan, lay, 1).any()
    assert not _bits(zero[2][off1:off1 + n1]).any()  # decodes to +0.0, not NaN from 0 / 0
    if ef:
        assert not _bits(zero[1][off1:off1 + n1]).any()  # the residual is g + r = +0.0
    # one non-finite element: the tensor decodes non-finite throughout, its neighbours as before
    for bad in (float("inf"), float("nan")):
        g = g0.clone()
        g[off1 + 3] = bad
        got = run(g, _resid("mix"))
        others_unaffected(got, bad)
        assert not bool(torch.isfinite(got[2][off1:off1 + n1]).any()), bad


# ---- 8. decode ----------------------------------------------------------------------------------
_DECODED = {}


def _rows(N, bits, levels):
    """(plan, layout, N payload rows encoded on the device, their decoded mean by the oracle),
    computed once per case and only read.  The ranks' gradients differ in magnitude (x 3^r), so
    the rank order of the fp32 sum matters."""
    if (N, bits) not in _DECODED:
        plan = _plan("edge")
        lay = Layout.build("qsgd", plan, bits)
        dp = ops.DevicePlan(plan, DEV)
        recv = torch.stack([_enc(dp, lay, levels, "l2" if r % 2 else "max",
                                 _bucket("edge", 10 + r) * 3.0 ** r, key=stream_key(SEED, 5, r))[0]
                            for r in range(N)])
        _DECODED[(N, bits)] = (plan, lay, recv, oracle.decode_sum(recv, plan, lay, levels, 1.0 / N))
    return _DECODED[(N, bits)]


@pytest.mark.parametrize("bits,levels", BITS, ids=BIT_IDS)
@pytest.mark.parametrize("N", [1, 2, 3, 8])
def test_decode_grad_out(N, bits, levels):
    ops.require()
    plan, lay, recv, mean = _rows(N, bits, levels)
    got = _dec(ops.DevicePlan(plan, DEV), lay, levels, recv, grad_scale=1.0 / N)
    own = _own(plan)
    for off, n in _ranges(plan):
        assert torch.equal(_bits(got[off:off + n]), _bits(mean[off:off + n])), off
        assert mean[off:off + n].any()
    assert bool(torch.isnan(got[~own]).all())  # nothing is written between the tensors


# lr = 2^-4 and dampening = 0 or 0.5: lr * d and (1 - dampening) * d are exact, so the reference
# does not depend on whether torch's CPU ``add_(x, alpha=)`` contracts its multiply-add (the kernels
# never do); every other step of oracle.sgd_apply is a separately rounded operation
HP = dict(lr=0.0625, momentum=0.9, dampening=0.0, weight_decay=5e-4)


def _check_apply(N, bits, levels, hp, first):
    plan, lay, recv, mean = _rows(N, bits, levels)
    gen = torch.Generator().manual_seed(11)
    p0 = torch.randn(plan.length, generator=gen)
    m0 = torch.randn(plan.length, generator=gen)
    p, m = p0.clone(), m0.clone()
    for off, n in _ranges(plan):
        oracle.sgd_apply(p[off:off + n], m[off:off + n], mean[off:off + n], first=first, **hp)
    assert not torch.equal(p, p0)
    pd, md = p0.clone().to(DEV), m0.clone().to(DEV)
    sh = torch.zeros(plan.length, dtype=torch.bfloat16, device=DEV)
    seed, step, rank = 5, 41, 3
    ks = torch.tensor([step, 0], dtype=torch.int32, device=DEV)
    lr_t = torch.tensor([hp["lr"]], device=DEV)  # the device scalar wins over the host value
    ops.qsgd_decode_apply(ops.DevicePlan(plan, DEV), recv.to(DEV), lay, levels, param=pd, mom=md,
                          grad_scale=1.0 / N, first=first, shadow=sh, key_state=ks, key_seed=seed,
                          key_rank=rank, lr_tensor=lr_t, **dict(hp, lr=999.0))
    assert torch.equal(_bits(pd.cpu()), _bits(p))  # the positions between tensors included
    assert torch.equal(_bits(md.cpu()), _bits(m))
    for off, n in _ranges(plan):
        assert torch.equal(sh[off:off + n].cpu(), p[off:off + n].to(torch.bfloat16))
    assert [int(v) & 0xFFFFFFFF for v in ks.cpu()] == [step + 1, stream_key(seed, step + 1, rank)]


@pytest.mark.parametrize("first", [True, False], ids=["first", "later"])
@pytest.mark.parametrize("nesterov", [True, False], ids=["nesterov", "heavy-ball"])
@pytest.mark.parametrize("bits,levels", BITS, ids=BIT_IDS)
@pytest.mark.parametrize("N", [1, 2, 3, 8])
def test_decode_apply_sgd(N, bits, levels, nesterov, first):
    ops.require()
    _check_apply(N, bits, levels, dict(HP, nesterov=nesterov), first)


@pytest.mark.parametrize("bits,levels", BITS, ids=BIT_IDS)
def test_decode_apply_sgd_with_dampening(bits, levels):
    ops.require()
    _check_apply(3, bits, levels, dict(HP, dampening=0.5, nesterov=False), False)


# ---- 9. unbiasedness under the L2 norm ----------------------------------------------------------
@pytest.mark.parametrize("bits,levels", BITS, ids=BIT_IDS)
def test_l2_unbiased_on_the_device(bits, levels):
    """A decoded element is step * (floor + Bernoulli(frac)) with step = |x|_2 / levels, so the
    mean over K keys has a standard deviation of at most step / (2 sqrt(K)).  The keys are
    counter-based and the outcome deterministic: the oracle's worst element sits at 3.6 of those
    units (tests/unit/test_compress.py), so 6 leaves room for the scale's last bits and none for a
    biased rounding.  Every element is held to it."""
    ops.require()
    plan = _plan(sim.UNBIASED)
    lay = Layout.build("qsgd", plan, bits)
    dp = ops.DevicePlan(plan, DEV)
    g = _bucket(sim.UNBIASED, sim.UNBIASED_SEED)
    acc = torch.zeros(plan.length, dtype=torch.float64)
    for key in sim.UNBIASED_KEYS:
        pay, _ = _enc(dp, lay, levels, "l2", g, key=key)
        acc += _dec(dp, lay, levels, pay[None]).double()
    worst = sim.worst_z(plan, g, acc / len(sim.UNBIASED_KEYS), levels)
    print(f"\nqsgd-l2-unbiased bits={bits} worst_z={worst:.3f}")
    assert worst <= sim.UNBIASED_Z


# ---- 10. graph capture --------------------------------------------------------------------------
@pytest.mark.parametrize("bits,levels,norm", [(8, 127, "l2"), (4, 7, "max")],
                         ids=["int8-l2", "int4-max"])
def test_encode_decode_graph_capture(bits, levels, norm):
    """Encode (error feedback, key from device memory) + decode-apply (key advance) captured on a
    side stream and replayed with fresh gradients copied into the static buffer: bitwise the eager
    run with host keys.  The second gradient is 1/8 of the first: a scratch left uncleared by a
    replay would show in its scale."""
    ops.require()
    plan = _plan("mix")
    lay = Layout.build("qsgd", plan, bits)
    dp = ops.DevicePlan(plan, DEV)
    hp = dict(lr=0.05, momentum=0.9, dampening=0.0, weight_decay=1e-4, nesterov=False)
    grads = [(_bucket("mix", 60 + i) * s).to(DEV) for i, s in enumerate((1.0, 0.125, 1.0))]
    p0 = torch.randn(plan.length, generator=torch.Generator().manual_seed(60)).to(DEV)

    def state():
        return dict(g=torch.zeros(plan.length, device=DEV), r=torch.zeros(plan.length, device=DEV),
                    p=p0.clone(), m=torch.zeros(plan.length, device=DEV),
                    pay=torch.zeros(1, lay.nbytes, dtype=torch.uint8, device=DEV))

    eager = state()
    for i, g in enumerate(grads):
        eager["g"].copy_(g)
        ops.qsgd_encode(dp, eager["g"], eager["pay"][0], lay, levels, norm,
                        stream_key(SEED, 1 + i, 0), resid=eager["r"])
        ops.qsgd_decode_apply(dp, eager["pay"], lay, levels, param=eager["p"], mom=eager["m"],
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
            ops.qsgd_encode(dp, cap["g"], cap["pay"][0], lay, levels, norm, 0, resid=cap["r"],
                            key_tensor=ks[1:2])
            ops.qsgd_decode_apply(dp, cap["pay"], lay, levels, param=cap["p"], mom=cap["m"],
                                  first=False, key_state=ks, key_seed=SEED, key_rank=0, **hp)
    torch.cuda.current_stream().wait_stream(side)
    graph.replay()  # capturing does not run: this is the first step
    for g in grads[1:]:
        cap["g"].copy_(g)
        graph.replay()
    torch.cuda.synchronize()
    for k in ("pay", "r", "p", "m"):
        assert torch.equal(_bits(cap[k]) if k != "pay" else cap[k],
                           _bits(eager[k]) if k != "pay" else eager[k]), k
    assert float(eager["r"].abs().max()) > 0
    assert [int(v) & 0xFFFFFFFF for v in ks.cpu()] == [4, stream_key(SEED, 4, 0)]


# ---- 11. refusals -------------------------------------------------------------------------------
@pytest.mark.parametrize("bits,levels", BITS, ids=BIT_IDS)
def test_bad_operands_rejected(bits, levels):
    """Checked on the host, before any launch: the payload and the residual keep their sentinel."""
    ops.require()
    plan = _plan("mix")
    lay = Layout.build("qsgd", plan, bits)
    dp = ops.DevicePlan(plan, DEV)
    g = _bucket("mix", 1).to(DEV)
    pay = torch.full((lay.nbytes,), SENT, dtype=torch.uint8, device=DEV)
    r = torch.full((plan.length,), R_GAP, device=DEV)
    with pytest.raises(ValueError):  # levels too large for the code width
        ops.qsgd_encode(dp, g, pay, lay, levels + 1, "max", KEY, resid=r)
    with pytest.raises(ValueError):  # payload shorter than the layout
        ops.qsgd_encode(dp, g, pay[:lay.nbytes - 16], lay, levels, "max", KEY, resid=r)
    with pytest.raises(ValueError):  # residual shorter than the bucket
        ops.qsgd_encode(dp, g, pay, lay, levels, "max", KEY, resid=r[:plan.length - 64])
    for kind in ("topk_qsgd", "tern", "sign"):  # another codec's offsets into the payload
        other = Layout.build(kind, plan, bits)
        big = torch.full((max(other.nbytes, lay.nbytes),), SENT, dtype=torch.uint8, device=DEV)
        with pytest.raises(ValueError):
            ops.qsgd_encode(dp, g, big, other, levels, "max", KEY, resid=r)
        assert bool((big == SENT).all())
    torch.cuda.synchronize()
    assert bool((pay == SENT).all()) and bool((r == R_GAP).all())
