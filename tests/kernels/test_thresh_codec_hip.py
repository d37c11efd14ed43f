"""The threshold-search sparsifier's HIP kernels (ops/csrc/thresh_codec.hip) vs the torch oracle, on
one MI355X.

Exactness contract: payload bytes (counts, indices, values, the zeroed unused slots and the
alignment pads), residuals, decoded sums, the fused SGD step and the key advance are bitwise the
oracle's, on the bucket of edge-case tensors that the CPU tests share (tests/thresh_sim.py), and
whatever the warm-start state holds."""
import pytest
import torch

from ewdml import ops
from ewdml.compress import oracle
from ewdml.compress.plan import BucketPlan, Layout
from ewdml.compress.rng import stream_key
from tests import thresh_sim as sim

pytestmark = pytest.mark.gpu

DEV = "cuda"


def _plan(numels=sim.NUMELS, ratio=sim.RATIO, dense_below=sim.DENSE_BELOW):
    offs, length = sim.offsets(numels)
    return BucketPlan(list(numels), offs, ratio, sim.BUCKET_OFFSET, length, dense_below)


def _bucket(seed):
    return torch.from_numpy(sim.bucket(seed))


def _resid0():
    """The residual before the first encode: finite everywhere (inf - inf has no one bit pattern)."""
    r = _bucket(1) * 0.25
    r[~torch.isfinite(r)] = 0.5
    return r


def _bits(t):
    return t.contiguous().view(torch.int32)


def _assert_same(got, ref, what, cast=False):
    """Bitwise -- but where both hold a NaN, its sign bit may differ.  The fused step's ``p - lr *
    d`` reaches the shared bucket's NaN gradient, and which sign the NaN of a subtraction carries
    is the adder's business (the host multiplies by ``-lr`` and adds, the GPU adds a negated
    operand): no code of the codec decides it.  Every other bit of every element is compared.
    ``cast``: the reference is torch's own fp32 -> bf16 cast, which writes a NaN as 0x7fff where the
    kernels' shared ``ew_f2bf`` keeps its top payload bits (0x7fc0): there a NaN matches a NaN."""
    got, ref = got.float(), ref.float()
    x = _bits(got) ^ _bits(ref)
    both_nan = torch.isnan(got) & torch.isnan(ref)
    bad = (x != 0) & ~both_nan
    print(f"{what}: {int((x != 0).sum())} words differ, {int(bad.sum())} of them outside NaNs, at "
          f"{bad.nonzero().flatten()[:8].tolist()}; NaNs {int(both_nan.sum())}")
    assert not bad.any(), what
    assert cast or ((x[both_nan] & 0x7FFFFFFF) == 0).all(), f"{what}: a NaN's payload differs"


_ENCODED = {}


def _reference(ef):
    """(plan, layout, [(gradient, payload, residual after it)] of two successive encodes), computed
    once per setting by the oracle and only read."""
    if ef not in _ENCODED:
        plan = _plan()
        lay = Layout.build("thresh", plan)
        r = _resid0() if ef else None
        steps = []
        for it in range(2):
            g = _bucket(2 * it)
            pay = oracle.encode_thresh(g.clone(), plan, lay, r)
            steps.append((g, pay, None if r is None else r.clone()))
        _ENCODED[ef] = (plan, lay, steps)
    return _ENCODED[ef]


def _check_encodes(ef, state, passes=None):
    plan, lay, steps = _reference(ef)
    dp = ops.DevicePlan(plan, DEV)
    pay = torch.full((lay.nbytes,), 0xFF, dtype=torch.uint8, device=DEV)
    r_dev = _resid0().to(DEV) if ef else None
    for it, (g, ref, r_ref) in enumerate(steps):
        ops.thresh_encode(dp, g.to(DEV), pay, lay, resid=r_dev, state=state, passes=passes)
        got = pay.cpu()
        C = plan.num_chunks
        gc = oracle._section(got, lay.counts, C, torch.int16)
        rc = oracle._section(ref, lay.counts, C, torch.int16)
        assert torch.equal(gc, rc), f"encode {it}: counts {gc.tolist()} vs {rc.tolist()}"
        assert torch.equal(got, ref), \
            f"encode {it}: payload differs at {(got != ref).nonzero()[:10].flatten()}"
        if ef:
            assert torch.equal(_bits(r_dev.cpu()), _bits(r_ref)), f"encode {it}: residual"
    return plan, lay


@pytest.mark.parametrize("ef", [False, True], ids=["plain", "ef"])
def test_encode_matches_oracle(ef):
    """Two encodes into the same buffers, the payload pre-filled with 0xFF so that an unwritten
    byte shows; a cold start (no state)."""
    ops.require()
    _check_encodes(ef, None)


@pytest.mark.parametrize("fill", ["zero", "top", "random"])
@pytest.mark.parametrize("ef", [False, True], ids=["plain", "ef"])
def test_encode_does_not_depend_on_the_search_state(ef, fill):
    """The warm-start state decides where the search starts and nothing else; afterwards it holds
    the thresholds, which the oracle's rule gives too."""
    ops.require()
    plan = _plan()
    C = plan.num_chunks
    if fill == "random":
        state = torch.randint(0, 32769, (C,), generator=torch.Generator().manual_seed(3),
                              dtype=torch.int32)
        state[0], state[1] = -7, 1 << 30  # out of range: clamped
    else:
        state = torch.full((C,), 0 if fill == "zero" else 32768, dtype=torch.int32)
    state = state.to(DEV)
    passes = torch.full((C,), -1, dtype=torch.int32, device=DEV)
    plan, lay = _check_encodes(ef, state, passes)
    g, _, r = _reference(ef)[2][1]
    acc = g if not ef else g + _reference(ef)[2][0][2]
    cap = plan.thresh_slots()[0]
    want = [oracle.thresh_threshold(oracle.thresh_level(
        acc[s:s + n].contiguous()), cap[c]) for c, (s, n) in
        enumerate(zip(plan.chunk_start, plan.chunk_len))]
    assert state.cpu().tolist() == want
    p = passes.cpu()
    print(f"thresh {fill} ef={ef}: passes of the second encode {p.tolist()}")
    assert int(p.min()) >= 0 and int(p.max()) <= 20


@pytest.mark.parametrize("ratio", [0.5, 1.0])
def test_encode_dense_chunks(ratio):
    """Chunks that send half or all of their elements: every thread writes, the compaction's
    offsets cross every wave and slab."""
    ops.require()
    plan = _plan([8192 * 2 + 77, 1000], ratio=ratio, dense_below=0)
    lay = Layout.build("thresh", plan)
    dp = ops.DevicePlan(plan, DEV)
    gen = torch.Generator().manual_seed(17)
    g = torch.zeros(plan.length)
    for o, n in zip(plan.offsets, plan.numels):
        g[o:o + n] = torch.randn(n, generator=gen)
    r_ref = torch.zeros(plan.length)
    r_dev = r_ref.to(DEV)
    pay = torch.full((lay.nbytes,), 0xFF, dtype=torch.uint8, device=DEV)
    ref = oracle.encode_thresh(g.clone(), plan, lay, r_ref)
    ops.thresh_encode(dp, g.to(DEV), pay, lay, resid=r_dev)
    assert torch.equal(pay.cpu(), ref)
    assert torch.equal(_bits(r_dev.cpu()), _bits(r_ref))
    counts = oracle._section(ref, lay.counts, plan.num_chunks, torch.int16).long() & 0xFFFF
    assert int(counts[0]) > 0.45 * 8192 * ratio


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_encode_from_per_tensor_pointers(dtype):
    """Autograd's own per-tensor gradients (fp32 or bf16, read through the pointer table) give the
    flat form's payload and residual; the gradients are not modified."""
    ops.require()
    plan = _plan()
    lay = Layout.build("thresh", plan)
    g = _bucket(0)
    for o, n in zip(plan.offsets, plan.numels):  # the flat reference holds the same values
        g[o:o + n] = g[o:o + n].to(dtype).float()
    dp = ops.DevicePlan(plan, DEV)
    grads = [g[o:o + n].clone().to(dtype).to(DEV) for o, n in zip(plan.offsets, plan.numels)]
    before = [t.clone() for t in grads]
    pay = torch.full((lay.nbytes,), 0xFF, dtype=torch.uint8, device=DEV)
    r_ref = _resid0()
    r_dev = r_ref.to(DEV)
    ref = oracle.encode_thresh(g.clone(), plan, lay, r_ref)
    ops.thresh_encode(dp, grads, pay, lay, resid=r_dev)
    assert torch.equal(pay.cpu(), ref)
    assert torch.equal(_bits(r_dev.cpu()), _bits(r_ref))
    for a, b in zip(grads, before):
        assert torch.equal(_bits(a.float()), _bits(b.float()))


# ---- decode ---------------------------------------------------------------------------------------
_DECODED = {}


def _rows(N):
    """(plan, layout, received rows, their decoded mean), computed once per N and only read.  The
    ranks' gradients differ in magnitude, so the rank order of the fp32 sum matters; their infs
    have one sign."""
    if N not in _DECODED:
        plan = _plan()
        lay = Layout.build("thresh", plan)
        recv = torch.stack([oracle.encode_thresh(_bucket(10 + 2 * r) * (3.0 ** (r % 4)), plan, lay)
                            for r in range(N)])
        _DECODED[N] = (plan, lay, recv, oracle.decode_sum(recv, plan, lay, 1, 1.0 / N))
    return _DECODED[N]


def _own(plan):
    own = torch.zeros(plan.length, dtype=torch.bool)
    for off, n in zip(plan.offsets, plan.numels):
        own[off:off + n] = True
    return own


@pytest.mark.parametrize("N", [1, 2, 3, 8])
def test_decode_grad_out(N):
    ops.require()
    plan, lay, recv, g = _rows(N)
    dp = ops.DevicePlan(plan, DEV)
    go = torch.full((plan.length,), 7.0, device=DEV)
    ops.thresh_decode_apply(dp, recv.to(DEV), lay, grad_out=go, grad_scale=1.0 / N)
    got = go.cpu()
    own = _own(plan)
    assert torch.equal(_bits(got[own]), _bits(g[own]))
    assert (got[~own] == 7.0).all()  # nothing is written between the tensors
    assert torch.nan_to_num(g[own], posinf=0.0).abs().max() > 0


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
    ops.thresh_decode_apply(dp, recv.to(DEV), lay, param=pd, mom=md, grad_scale=1.0 / N,
                            first=first, shadow=sh, key_state=ks, key_seed=seed, key_rank=rank,
                            lr_tensor=lr_t, **dict(hp, lr=999.0))
    _assert_same(pd.cpu(), p, "parameters")  # the positions between tensors included
    _assert_same(md.cpu(), m, "momentum")
    own = _own(plan)
    _assert_same(sh.cpu()[own], p[own].to(torch.bfloat16), "bf16 shadow", cast=True)
    assert [int(v) & 0xFFFFFFFF for v in ks.cpu()] == [step + 1, stream_key(seed, step + 1, rank)]


def test_decode_clamps_a_corrupt_row():
    """A row whose every count is 0xFFFF and whose indices reach past their chunks decodes as the
    oracle's clamped rule does: the chunk's own slots and no further, an index at or past the
    chunk's length dropped.  Nothing outside the chunk's tile is touched."""
    ops.require()
    plan, lay, recv, _ = _rows(2)
    cap, slot0, S = plan.thresh_slots()
    bad = recv.clone()
    counts = oracle._section(bad[1], lay.counts, plan.num_chunks, torch.int16)
    idx = oracle._section(bad[1], lay.idx, S, torch.int16)
    vals = oracle._section(bad[1], lay.codes, S, torch.float32)
    counts[:] = -1
    idx[slot0[3]] = 5  # the five-element chunk's one slot
    c = plan.tensor_chunk0[sim.CUBED_T] + 1  # 808 elements, 9 slots
    idx[slot0[c]:slot0[c] + 9] = torch.tensor([0, 807, 808, 8191, -1, 1, 2, 3, 4],
                                              dtype=torch.int16)
    vals[slot0[c]:slot0[c] + 9] = torch.arange(1.0, 10.0)
    ref = oracle.decode_sum(bad, plan, lay, 1, 0.5)
    dp = ops.DevicePlan(plan, DEV)
    go = torch.full((plan.length,), 7.0, device=DEV)
    ops.thresh_decode_apply(dp, bad.to(DEV), lay, grad_out=go, grad_scale=0.5)
    got = go.cpu()
    own = _own(plan)
    assert torch.equal(_bits(got[own]), _bits(ref[own]))
    assert (got[~own] == 7.0).all()


def test_kernels_use_no_scratch():
    """The loaded code objects' resource report: no private (scratch) memory in any of the three
    kernels, a 32 KiB tile in the decode and a few words of LDS in the encode."""
    ops.require()
    info = ops.thresh_kernel_info()
    print(f"thresh kernels: {info}")
    assert set(info) == {"k_thr_encode<EF>", "k_thr_encode", "k_thr_decode_apply"}
    for name, v in info.items():
        assert v["scratch_bytes"] == 0, f"{name} uses {v['scratch_bytes']} bytes of scratch"
    assert info["k_thr_decode_apply"]["lds_bytes"] == 32768
    assert info["k_thr_encode<EF>"]["lds_bytes"] <= 256


def test_bad_operands_rejected():
    """Size, dtype, alignment and the layout are checked on the host, before any launch."""
    ops.require()
    plan = _plan([1000, 8192 + 1])
    lay = Layout.build("thresh", plan)
    dp = ops.DevicePlan(plan, DEV)
    g = torch.zeros(plan.length, device=DEV)
    pay = torch.zeros(lay.nbytes, dtype=torch.uint8, device=DEV)
    bigpay = torch.zeros(lay.nbytes + 16, dtype=torch.uint8, device=DEV)
    with pytest.raises(ValueError):  # payload too short
        ops.thresh_encode(dp, g, pay[:lay.nbytes - 16], lay)
    with pytest.raises(ValueError):  # gradient too short
        ops.thresh_encode(dp, g[:100], pay, lay)
    with pytest.raises(TypeError):
        ops.thresh_encode(dp, g, pay, lay, resid=g.to(torch.bfloat16))
    with pytest.raises(ValueError):  # misaligned view
        ops.thresh_encode(dp, g, bigpay[4:], lay)
    with pytest.raises(ValueError):  # a state that is too short
        ops.thresh_encode(dp, g, pay, lay, state=torch.zeros(1, dtype=torch.int32, device=DEV))
    with pytest.raises(ValueError):  # another codec's layout, another plan's layout
        ops.thresh_encode(dp, g, pay, Layout.build("topk", plan))
    with pytest.raises(ValueError):
        ops.thresh_encode(dp, g, pay, Layout.build("thresh", _plan([1000, 8192 + 1, 64])))
    with pytest.raises(ValueError):  # row length is not the layout's
        ops.thresh_decode_apply(dp, bigpay[None], lay, grad_out=g)
    with pytest.raises(ValueError):  # nothing to do
        ops.thresh_decode_apply(dp, pay[None], lay)
    torch.cuda.synchronize()
    assert not pay.any() and not g.any()  # nothing ran
