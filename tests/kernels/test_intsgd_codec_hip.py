"""The IntSGD codec's HIP kernels (ops/csrc/intsgd_codec.hip) vs the torch oracle, on one MI355X.

Exactness contract: payload bytes (codes and the zero pads), residuals, saturation counts, the
fused SGD step with its bf16 shadow and key advance, the per-row update partials and the scale
state are bitwise the oracle's, on the bucket of edge-case tensors that the CPU tests share
(tests/intsgd_sim.py)."""
import numpy as np
import pytest
import torch

from ewdml import ops
from ewdml.compress import oracle
from ewdml.compress.codecs import IntSGDState
from ewdml.compress.plan import BucketPlan, Layout
from ewdml.compress.rng import stream_key
from tests import intsgd_sim as sim

pytestmark = pytest.mark.gpu

DEV = "cuda"
SEED = 3


def _plan():
    offs, length = sim.offsets()
    return BucketPlan(list(sim.NUMELS), offs, 1.0, sim.BUCKET_OFFSET, length)


def _bits(t):
    return t.contiguous().view(torch.int32)


def _state(alpha, inv_a=None, inv_na=None, world=1):
    st = IntSGDState(DEV)
    a = np.float32(alpha)
    if a != 0:
        inv_a = np.float32(1.0 / float(a)) if inv_a is None else inv_a
        inv_na = np.float32(1.0 / (float(a) * world)) if inv_na is None else inv_na
    else:
        inv_a = inv_na = 0.0
    st.load(dict(r=1.0, alpha=float(a), inv_a=float(inv_a), inv_na=float(inv_na), steps=1))
    return st


@pytest.mark.parametrize("world", [1, 3, 8, 127])
@pytest.mark.parametrize("ef", [False, True], ids=["plain", "ef"])
def test_encode_matches_oracle(ef, world):
    """Two encodes into the same buffers (the second with the next step's key and another
    gradient), the payload pre-filled with 0xFF so that an unwritten byte shows."""
    ops.require()
    plan, q = _plan(), sim.q_of(world)
    lay = Layout.build("intsgd", plan)
    dp = ops.DevicePlan(plan, DEV)
    st = _state(sim.ALPHA, world=world)
    v = st.values()
    pay = torch.full((lay.nbytes,), 0xFF, dtype=torch.uint8, device=DEV)
    sat = torch.full((plan.num_chunks,), -1, dtype=torch.int32, device=DEV)
    r_ref = torch.from_numpy(sim.bucket(1, q)) * 0.25 if ef else None
    if ef:  # the residual of a non-finite element stays non-finite: start from finite values
        r_ref = torch.nan_to_num(r_ref, nan=0.0, posinf=0.0, neginf=0.0)
    r_dev = r_ref.to(DEV) if ef else None
    total = 0
    for it in range(2):
        g = torch.from_numpy(sim.bucket(2 * it, q))
        key = stream_key(SEED, 7 + it, 1)
        ref, sref = oracle.encode_intsgd(g.clone(), plan, lay, v["alpha"], v["inv_a"], q, key, r_ref)
        ops.int_encode(dp, g.to(DEV), pay, lay, st.buf, sat, q, key, resid=r_dev)
        got = pay.cpu()
        assert torch.equal(got, ref), \
            f"encode {it}: payload differs at {(got != ref).nonzero()[:10].flatten()}"
        assert torch.equal(sat.cpu(), sref), f"encode {it}: saturation counts"
        if ef:
            assert torch.equal(_bits(r_dev.cpu()), _bits(r_ref)), f"encode {it}: residual"
        total += int(sref.sum())
    assert total > 0 and int(got.view(torch.int8).abs().max()) == q  # the bucket does its job


@pytest.mark.parametrize("ef", [False, True], ids=["plain", "ef"])
def test_encode_alpha_zero(ef):
    """lr 0: alpha and both inverses are 0 and every code of a finite element is 0."""
    ops.require()
    plan = _plan()
    lay = Layout.build("intsgd", plan)
    dp = ops.DevicePlan(plan, DEV)
    st = _state(0.0)
    pay = torch.full((lay.nbytes,), 0xFF, dtype=torch.uint8, device=DEV)
    sat = torch.zeros(plan.num_chunks, dtype=torch.int32, device=DEV)
    g = torch.from_numpy(sim.bucket(0, 15))
    r_ref = torch.from_numpy(sim.bucket(3, 15) * np.float32(0.5)) if ef else None
    if ef:
        r_ref = torch.nan_to_num(r_ref, nan=0.0, posinf=0.0, neginf=0.0)
    r_dev = r_ref.to(DEV) if ef else None
    key = stream_key(SEED, 2, 0)
    ref, sref = oracle.encode_intsgd(g.clone(), plan, lay, 0.0, 0.0, 15, key, r_ref)
    ops.int_encode(dp, g.to(DEV), pay, lay, st.buf, sat, 15, key, resid=r_dev)
    assert torch.equal(pay.cpu(), ref) and torch.equal(sat.cpu(), sref)
    assert int(ref.view(torch.int8).abs().max()) == 0
    if ef:
        assert torch.equal(_bits(r_dev.cpu()), _bits(r_ref))


def test_key_from_device_memory():
    ops.require()
    plan = _plan()
    lay = Layout.build("intsgd", plan)
    dp = ops.DevicePlan(plan, DEV)
    st = _state(sim.ALPHA)
    g = torch.from_numpy(sim.bucket(0, 15)).to(DEV)
    key = stream_key(SEED, 12, 2)
    ks = torch.tensor([12, key - (1 << 32) if key >= 1 << 31 else key], dtype=torch.int32,
                      device=DEV)
    out = []
    for kw in (dict(key=key), dict(key=0x5A5A5A5A, key_tensor=ks[1:2])):  # the device key wins
        pay = torch.full((lay.nbytes,), 0xFF, dtype=torch.uint8, device=DEV)
        sat = torch.zeros(plan.num_chunks, dtype=torch.int32, device=DEV)
        ops.int_encode(dp, g, pay, lay, st.buf, sat, 15, **kw)
        out.append(pay.cpu())
    assert torch.equal(out[0], out[1])


def _summed(plan, lay, world, q, v):
    """The sum of ``world`` oracle encodes built on the host, with the bytes 0x7F, 0x81 and 0x80
    placed by hand on elements of the last tensor."""
    tot = torch.zeros(lay.nbytes, dtype=torch.int32)
    for rk in range(world):
        g = torch.from_numpy(sim.bucket(10 + rk, q))
        pay, _ = oracle.encode_intsgd(g, plan, lay, v["alpha"], v["inv_a"], q,
                                      stream_key(SEED, 5, rk))
        tot += pay.view(torch.int8).to(torch.int32)
    assert int(tot.abs().max()) <= 127
    s = tot.to(torch.int8).view(torch.uint8).clone()
    o = plan.offsets[-1]
    s[o + 3], s[o + 4], s[o + 8195] = 0x7F, 0x81, 0x80
    return s


@pytest.mark.parametrize("world", [1, 8])
@pytest.mark.parametrize("first", [True, False], ids=["first", "later"])
@pytest.mark.parametrize("momentum", [0.0, 0.9])
def test_decode_apply_matches_oracle(momentum, first, world):
    ops.require()
    plan, q = _plan(), sim.q_of(world)
    lay = Layout.build("intsgd", plan)
    dp = ops.DevicePlan(plan, DEV)
    st = _state(sim.ALPHA, world=world)
    v = st.values()
    summed = _summed(plan, lay, world, q, v)
    gen = torch.Generator().manual_seed(11)
    p_ref = torch.randn(plan.length, generator=gen)
    m_ref = torch.randn(plan.length, generator=gen) * 0.1
    p_dev, m_dev = p_ref.to(DEV), m_ref.to(DEV)
    shadow = torch.zeros(plan.length, dtype=torch.bfloat16, device=DEV)
    part_ref = torch.zeros(plan.num_chunks)
    part_dev = torch.full((plan.num_chunks,), -1.0, device=DEV)
    # lr = 2^-4: lr * d is exact, so the reference does not depend on whether torch's CPU
    # ``add_(x, alpha=)`` contracts its multiply-add (the kernels never do)
    hp = dict(lr=0.0625, momentum=momentum, dampening=0.0, weight_decay=1e-4, nesterov=momentum > 0)
    lr_t = torch.tensor([hp["lr"]], dtype=torch.float32, device=DEV)
    ks = torch.tensor([4, 0], dtype=torch.int32, device=DEV)
    prev_dev = p_dev.clone()
    oracle.intsgd_apply(summed, plan, lay, v["inv_na"], p_ref, m_ref, hp, first, part_ref)
    ops.int_decode_apply(dp, summed.to(DEV), lay, st.buf, part_dev, p_dev, m_dev, lr=123.0,
                         momentum=momentum, dampening=0.0, weight_decay=1e-4,
                         nesterov=momentum > 0, first=first, shadow=shadow, key_state=ks,
                         key_seed=SEED, key_rank=2, lr_tensor=lr_t)
    assert torch.equal(_bits(p_dev.cpu()), _bits(p_ref))
    assert torch.equal(_bits(m_dev.cpu()), _bits(m_ref))
    own = oracle._mx_mask(plan, "cpu")
    assert torch.equal(shadow.cpu()[own].view(torch.int16),
                       p_ref.to(torch.bfloat16)[own].view(torch.int16))
    key = stream_key(SEED, 5, 2)
    assert ks.cpu().tolist() == [5, key - (1 << 32) if key >= 1 << 31 else key]
    assert torch.equal(_bits(part_dev.cpu()), _bits(part_ref))
    # the stand-alone norm launch gives the fused partials bit for bit
    part2 = torch.full((plan.num_chunks,), -1.0, device=DEV)
    ops.int_update_norm(dp, p_dev, prev_dev, part2)
    assert torch.equal(_bits(part2.cpu()), _bits(part_dev.cpu()))
    assert float(part_ref.sum()) > 0


def test_alpha_matches_oracle_over_three_steps():
    ops.require()
    st = IntSGDState(DEV)
    lr_t = torch.tensor([0.01], dtype=torch.float32, device=DEV)
    ref = dict(r=0.0, steps=0)
    gen = torch.Generator().manual_seed(5)
    for it, n in enumerate((1, 1500, 2049)):  # one row, more than a tile, more than two
        part = (torch.rand(n, generator=gen) * 1e-6).to(torch.float32)
        ref = oracle.intsgd_alpha(part, ref["r"], ref["steps"], 0.01, 1234567, 3)
        ops.int_alpha(part.to(DEV), st.buf, 99.0, 1234567, 3, lr_tensor=lr_t)
        got = st.values()
        for k in IntSGDState.FIELDS:
            a, b = np.float64(got[k]), np.float64(ref[k])
            assert a.tobytes() == b.tobytes(), f"step {it}: {k} {got[k]!r} vs {ref[k]!r}"
    # lr 0: alpha and both inverses are 0
    ops.int_alpha(part.to(DEV), st.buf, 0.0, 1234567, 3)
    got = st.values()
    assert got["alpha"] == 0.0 and got["inv_a"] == 0.0 and got["inv_na"] == 0.0
