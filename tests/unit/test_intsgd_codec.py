"""IntSGD on the CPU (compress/oracle.py encode_intsgd / intsgd_apply / intsgd_alpha): the oracle
against the independent numpy simulation (tests/intsgd_sim.py) bit for bit, the codec's exact
properties, the scale rule against fp64 numpy, and the codec object, the Horovod-style constructor
and the command line."""
import math

import numpy as np
import pytest
import torch

import ewdml
from ewdml.compress import oracle
from ewdml.compress.codecs import Codec
from ewdml.compress.plan import BucketPlan, Layout
from tests import intsgd_sim as sim

SEED = 3


def _plan():
    offs, length = sim.offsets()
    return BucketPlan(list(sim.NUMELS), offs, 1.0, sim.BUCKET_OFFSET, length)


def _bits(a):
    return np.asarray(a, dtype=np.float32).view(np.int32)


def test_layout_and_ratio():
    plan = _plan()
    lay = Layout.build("intsgd", plan)
    assert lay.nbytes == plan.length and lay.codes == 0 and lay.bits == 8
    c = Codec("intsgd").bind_intsgd([plan], "cpu", 8)
    assert c.describe() == "intsgd8" and c.q == 15
    assert 4 * plan.numel / lay.nbytes == pytest.approx(4 * sum(sim.NUMELS) / plan.length)
    with pytest.raises(ValueError, match="packed at multiples of 64"):
        Layout.build("intsgd", BucketPlan([10, 10], [0, 16], 1.0, 0, 64))
    with pytest.raises(ValueError, match="bound by its own exchange"):
        Codec("intsgd").bind([plan], "cpu")


@pytest.mark.parametrize("world,q", sorted(sim.WORLDS.items()))
@pytest.mark.parametrize("ef", [False, True], ids=["plain", "ef"])
def test_oracle_matches_simulation(ef, world, q):
    """Payload, residual and saturation counts, over two steps into the same residual."""
    assert oracle.intsgd_q(world) == q == sim.q_of(world)
    plan = _plan()
    lay = Layout.build("intsgd", plan)
    offs, _ = sim.offsets()
    alpha, inv_a = sim.ALPHA, 1.0 / sim.ALPHA
    r0 = np.nan_to_num(sim.bucket(1, q) * np.float32(0.25), nan=0.0, posinf=0.0, neginf=0.0)
    r_o = torch.from_numpy(r0.copy()) if ef else None
    r_s = r0.copy() if ef else None
    for it in range(2):
        g = sim.bucket(2 * it, q)
        key = sim.stream_key(SEED, 7 + it, 1)
        pay, sat = oracle.encode_intsgd(torch.from_numpy(g.copy()), plan, lay, alpha, inv_a, q,
                                        key, r_o)
        codes, ssat = sim.encode(g, offs, sim.NUMELS, sim.BUCKET_OFFSET, alpha, inv_a, q, key, r_s)
        assert np.array_equal(pay.view(torch.int8).numpy(), codes), f"step {it}"
        assert np.array_equal(sat.numpy(), ssat), f"step {it}"
        assert int(ssat.sum()) > 0
        if ef:
            assert np.array_equal(_bits(r_o.numpy()), _bits(r_s)), f"step {it}"


def test_exact_properties():
    plan = _plan()
    lay = Layout.build("intsgd", plan)
    q = 15
    g = torch.from_numpy(sim.bucket(0, q))
    for key in (1, 2, 3):
        pay, sat = oracle.encode_intsgd(g, plan, lay, sim.ALPHA, 1.0 / sim.ALPHA, q, key)
        c = pay.view(torch.int8)
        # pads are 0 and every code lies in [-q, q]
        assert int(c[~oracle._mx_mask(plan, "cpu")].abs().max()) == 0 and int(c.abs().max()) == q
        o, n = plan.offsets[sim.INT_T], sim.NUMELS[sim.INT_T]
        want = torch.clamp(torch.round(g[o:o + n] * sim.ALPHA), -q, q).to(torch.int8)
        assert torch.equal(c[o:o + n], want)  # an integer y does not move, whatever the key
        o = plan.offsets[sim.WILD_T]
        assert c[o + 7] == 0 and c[o + 8] == q and c[o + 9] == -q  # NaN, +inf, -inf
        assert c[o + 5] == q and c[o + 6] == -q and c[o + 8190] == q
        o, n = plan.offsets[sim.ZERO_T], sim.NUMELS[sim.ZERO_T]
        assert int(c[o:o + n].abs().max()) == 0


def test_unbiased():
    """The mean of 4096 encodes of one value under different keys: a code is f + Bernoulli(p)
    with p = y - f, so the mean of K of them has standard error sqrt(p (1 - p) / K) <= 0.5 /
    sqrt(K) code units, and the decoded mean lies within 4 of them of the value."""
    K, alpha, q = 4096, 64.0, 15
    plan = BucketPlan([64], [0], 1.0, 0, 64)
    lay = Layout.build("intsgd", plan)
    vals = torch.linspace(-0.2, 0.2, 64)
    tot = torch.zeros(64, dtype=torch.float64)
    for k in range(K):
        pay, _ = oracle.encode_intsgd(vals, plan, lay, alpha, 1.0 / alpha, q,
                                      sim.stream_key(SEED, k, 0))
        tot += pay.view(torch.int8).to(torch.float64)
    y = (vals * alpha).double()
    p = y - torch.floor(y)
    se = torch.sqrt(p * (1 - p) / K)
    assert bool(((tot / K - y).abs() <= 4 * se + 1e-12).all())


@pytest.mark.parametrize("world,q", sorted(sim.WORLDS.items()))
def test_sum_stays_in_int8(world, q):
    plan = BucketPlan([64], [0], 1.0, 0, 64)
    lay = Layout.build("intsgd", plan)
    for sign in (1.0, -1.0):
        g = torch.full((64,), sign * 1e3)
        tot = torch.zeros(64, dtype=torch.int32)
        for rk in range(world):
            pay, sat = oracle.encode_intsgd(g, plan, lay, 64.0, 1 / 64.0, q, rk)
            assert int(sat.sum()) == 64
            tot += pay.view(torch.int8).to(torch.int32)
        assert int(tot.abs().max()) == world * q <= 127


def test_apply_and_partials_match_simulation():
    plan = _plan()
    lay = Layout.build("intsgd", plan)
    offs, L = sim.offsets()
    rs = np.random.RandomState(9)
    summed = rs.randint(-127, 128, size=L).astype(np.int8)
    o = offs[-1]
    summed.view(np.uint8)[[o + 3, o + 4, o + 8195]] = (0x7F, 0x81, 0x80)
    p0 = rs.standard_normal(L).astype(np.float32)
    m0 = (rs.standard_normal(L) * 0.1).astype(np.float32)
    inv_na = float(np.float32(1.0 / (64.0 * 3)))
    for momentum, first in ((0.0, False), (0.9, True), (0.9, False)):
        p_o, m_o = torch.from_numpy(p0.copy()), torch.from_numpy(m0.copy())
        p_s, m_s = p0.copy(), m0.copy()
        part = torch.zeros(plan.num_chunks)
        # lr = 2^-4: lr * d is exact, so the reference does not depend on whether torch's CPU
        # ``add_(x, alpha=)`` contracts its multiply-add (the simulation and the kernels never do)
        hp = dict(lr=0.0625, momentum=momentum, dampening=0.0, weight_decay=0.0, nesterov=False)
        oracle.intsgd_apply(torch.from_numpy(summed.view(np.uint8).copy()), plan, lay, inv_na,
                            p_o, m_o, hp, first, part)
        sp = sim.apply(summed, p_s, m_s, offs, sim.NUMELS, inv_na, 0.0625, momentum, first=first)
        assert np.array_equal(_bits(p_o.numpy()), _bits(p_s))
        assert np.array_equal(_bits(m_o.numpy()), _bits(m_s))
        assert np.array_equal(_bits(part.numpy()), _bits(sp))
        assert np.array_equal(_bits(oracle.intsgd_update_partials(
            p_o, torch.from_numpy(p0), plan).numpy()), _bits(sp))
    i = o + 8195  # the byte 0x80 decodes as -128
    assert p_o[i] != p0[i]


def test_alpha_rule_against_fp64():
    d, N, lr = 431080, 3, 0.01
    rs = np.random.RandomState(2)
    st = dict(r=0.0, steps=0)
    r = None
    for k in range(3):
        part = torch.from_numpy((rs.rand(300) * 1e-7).astype(np.float32))
        st = oracle.intsgd_alpha(part, st["r"], st["steps"], lr, d, N)
        S = 0.0
        for v in part.double().numpy():
            S += float(v)
        r = S if k == 0 else 0.9 * r + (1 - 0.9) * S
        assert st["r"] == r and st["s_last"] == S and st["steps"] == k + 1
        alpha = np.float32(float(np.float32(lr)) * math.sqrt(d) / math.sqrt(2 * N * r + 1e-16))
        assert st["alpha"] == float(alpha)
        assert st["inv_a"] == float(np.float32(1.0 / np.float64(alpha)))
        assert st["inv_na"] == float(np.float32(1.0 / (np.float64(alpha) * N)))
        assert sim.alpha_rule(part.numpy(), 0.0 if k == 0 else r_prev, k, lr, d, N) == (
            r, alpha, np.float32(st["inv_a"]), np.float32(st["inv_na"]))
        r_prev = r
    z = oracle.intsgd_alpha(part, st["r"], st["steps"], 0.0, d, N)
    assert z["alpha"] == 0.0 and z["inv_a"] == 0.0 and z["inv_na"] == 0.0


# ---- command line ---------------------------------------------------------------------------------
def _resolve(*flags):
    return ewdml.parse_args(["--compress", "intsgd", *flags]).resolved()


def test_cli():
    c = _resolve()
    assert c.error_feedback is False and c.hip_graph == "split"
    assert _resolve("--error-feedback").error_feedback is True
    assert _resolve("--no-error-feedback").error_feedback is False
    # what the benchmark always passes is accepted (and unused)
    c = _resolve("--qsgd-bits", "4", "--qsgd-levels", "7", "--error-feedback", "--ef-warmup",
                 "none", "--momentum", "0.9")
    assert c.error_feedback is True and c.topk_warmup == ""
    assert _resolve("--hip-graph", "split").hip_graph == "split"
    assert _resolve("--hip-graph", "off").hip_graph == "off"
    assert _resolve("--clip-grad-norm", "1.0").clip_grad_norm == 1.0


@pytest.mark.parametrize("flags,reason", [
    (["--optimizer", "adam"], "--optimizer sgd"),
    (["--optimizer", "lars"], "--optimizer sgd"),
    (["--optimizer", "lamb"], "--optimizer sgd"),
    (["--optimizer", "lion"], "--optimizer sgd"),
    (["--topology", "ps"], "--topology ps"),
    (["--topology", "sharded"], "--topology sharded"),
    (["--topology", "twostage"], "--topology twostage"),
    (["--sync-every", "4"], "--sync-every"),
    (["--select-best"], "--select-best"),
    (["--predivide", "2"], "--predivide"),
    (["--ef-mode", "plain"], "--ef-mode plain"),
    (["--hip-graph", "full"], "--hip-graph full"),
    (["--hip-graph", "segmented"], "--hip-graph segmented"),
])
def test_cli_refusals(flags, reason):
    with pytest.raises(ValueError, match="--compress intsgd .*" + reason):
        _resolve(*flags)


def test_other_refusals():
    from ewdml.config import Config
    from ewdml.parallel.horovod import Compression

    with pytest.raises(SystemExit):  # the pull codecs' choices stay as they were
        ewdml.parse_args(["--topology", "ps", "--pull-compress", "intsgd"])
    with pytest.raises(ValueError, match="--pull-compress intsgd"):
        Config(topology="ps", compress="qsgd", pull_compress="intsgd").resolved()
    with pytest.raises(ValueError, match="--compress intsgd has no parameter-server form"):
        Config(compress="intsgd", optimizer="sgd", pull_compress="qsgd").resolved()
    with pytest.raises(ValueError, match="--sign-rotate hadamard rotates the sign codec"):
        _resolve("--sign-rotate", "hadamard")
    with pytest.raises(ValueError, match="at most 127 ranks"):
        oracle.intsgd_q(128)
    assert Compression.intsgd().kind == "intsgd"


def test_distributed_optimizer_refuses_intsgd():
    from ewdml.parallel import horovod as hvd

    model = torch.nn.Linear(4, 2)
    with pytest.raises(ValueError, match="Compression.intsgd is not supported by "
                                         "DistributedOptimizer: the wrapped optimizer owns the step"):
        hvd.DistributedOptimizer(torch.optim.SGD(model.parameters(), lr=0.1),
                                 compression=hvd.Compression.intsgd())


def test_exchange_refusals():
    """The exchange's own checks: a non-fusable optimizer, another codec, and no health keys
    before the first scale exists."""
    from ewdml.compress import make_codec
    from ewdml.optim.flat import FlatSGD, make_optimizer
    from ewdml.parallel.comm import Comm
    from ewdml.parallel.intsgd import IntSGDExchange

    flat = sim.make_flat()
    with pytest.raises(ValueError, match="it needs --optimizer sgd"):
        IntSGDExchange(flat, Comm(), make_codec("intsgd"), make_optimizer("adam", flat, lr=1e-3))
    with pytest.raises(ValueError, match="needs --compress intsgd"):
        IntSGDExchange(flat, Comm(), make_codec("qsgd"), FlatSGD(flat, lr=0.1))
    ex = IntSGDExchange(flat, Comm(), make_codec("intsgd"), FlatSGD(flat, lr=0.1))
    assert ex.dense_step and ex.codec_health() == {} and ex.state() is None
    assert ex.bytes_per_step().payload_bytes == 4 * flat.numel


def test_predicted_as_qsgd():
    from ewdml.parallel.engine import plan_graph_mode

    kw = dict(model="VGG11", dtype="fp32")
    for world in (1, 8):
        q = plan_graph_mode(world, "rccl-stream", "qsgd", 9_231_114, 8, **kw)
        p = plan_graph_mode(world, "rccl-stream", "intsgd", 9_231_114, **kw)
        assert p["mode"] == "split" and p["wire_bytes"] == int(2 * (world - 1) / world * 9_231_114)
        assert q.get("predicted_ms") is not None and p["predicted_ms"] == q["predicted_ms"]
