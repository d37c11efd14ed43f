"""The TernGrad oracle (compress/oracle.py encode_tern, tern_scale, decode_sum) against an
independent numpy simulation (tests/tern_sim.py), against QSGD at one level, and against the
codec's own properties: the clipped scaler, unbiasedness without clipping, the error-feedback
identity, the payload size; then the codec object and the command line."""
import numpy as np
import pytest
import torch

import ewdml
from ewdml.compress import oracle
from ewdml.compress.codecs import Codec
from ewdml.compress.plan import BucketPlan, Layout, _align
from ewdml.parallel.engine import plan_graph_mode
from tests import tern_sim as sim

CLIPS = [2.5, 0.0]
KEY = sim.stream_key(3, 7, 1)


def _plan(numels=sim.NUMELS, bucket_offset=sim.BUCKET_OFFSET):
    offs, length = sim.offsets(numels)
    return BucketPlan(list(numels), offs, 1.0, bucket_offset, length)


@pytest.fixture(scope="module")
def shared():
    """The shared bucket, its plan and layout, and the oracle's and the simulation's encodes at
    both clips, without and with a residual: computed once, never modified."""
    plan = _plan()
    lay = Layout.build("tern", plan)
    g = sim.bucket(0)
    r0 = (sim.bucket(1) * np.float32(0.25)).astype(np.float32)
    out = {"plan": plan, "lay": lay, "g": g, "r0": r0}
    for clip in CLIPS:
        out["o", clip, False] = (oracle.encode_tern(torch.from_numpy(g), plan, lay, clip, KEY),
                                 None)
        res = torch.from_numpy(r0.copy())
        out["o", clip, True] = (oracle.encode_tern(torch.from_numpy(g), plan, lay, clip, KEY, res),
                                res)
        out["s", clip, False] = sim.encode(g, sim.NUMELS, plan.offsets, plan.bucket_offset, clip,
                                           KEY)
        out["s", clip, True] = sim.encode(g, sim.NUMELS, plan.offsets, plan.bucket_offset, clip,
                                          KEY, r0)
    return out


def test_rng_matches():
    from ewdml.compress import rng

    assert sim.stream_key(3, 7, 1) == rng.stream_key(3, 7, 1)
    idx = torch.tensor([0, 1, 4096, 2 ** 31 + 5, 2 ** 32 - 1])
    got = rng.uniform(idx, KEY)
    assert [float(x) for x in got] == [float(sim.uniform(int(i), KEY)) for i in idx]


@pytest.mark.parametrize("ef", [False, True])
@pytest.mark.parametrize("clip", CLIPS)
def test_payload_bytewise_against_sim(shared, clip, ef):
    pay, res = shared["o", clip, ef]
    spay, _, sres = shared["s", clip, ef]
    assert pay.numel() == spay.size == shared["lay"].nbytes
    assert np.array_equal(pay.numpy(), spay)
    if ef:
        assert np.array_equal(res.numpy().view(np.int32), sres.view(np.int32))


@pytest.mark.parametrize("clip", CLIPS)
def test_decode_against_sim(shared, clip):
    plan, lay = shared["plan"], shared["lay"]
    pays = [shared["o", clip, False][0], shared["o", clip, True][0]]
    got = oracle.decode_sum(torch.stack(pays), plan, lay, 1, 0.5)
    want = sim.decode_mean([p.numpy() for p in pays], sim.NUMELS, plan.offsets, plan.length, 0.5)
    assert np.array_equal(got.numpy().view(np.int32), want.view(np.int32))
    codes = oracle._unpack2(oracle._section(pays[0], lay.codes, plan.total_codes // 16,
                                            torch.int32))
    assert set(codes.tolist()) <= {-1, 0, 1}  # the code 2 is never written


def test_codes_equal_qsgd_at_one_level(shared):
    """Without clipping the codec is QSGD at one level with the max norm, code for code."""
    plan, g = shared["plan"], torch.from_numpy(shared["g"])
    qlay = Layout.build("qsgd", plan, 8)
    qpay = oracle.encode_qsgd(g, plan, qlay, 1, "max", KEY)
    q = oracle._section(qpay, qlay.codes, plan.total_codes, torch.int8).to(torch.int32)
    lay = shared["lay"]
    pay = shared["o", 0.0, False][0]
    t = oracle._unpack2(oracle._section(pay, lay.codes, plan.total_codes // 16, torch.int32))
    assert torch.equal(q, t)
    T = plan.num_tensors
    assert torch.equal(oracle._section(qpay, qlay.scales, T, torch.float32),
                       oracle._section(pay, lay.scales, T, torch.float32))


def test_scaler(shared):
    plan, lay, g = shared["plan"], shared["lay"], shared["g"]
    T = plan.num_tensors
    sc = oracle._section(shared["o", 2.5, False][0], lay.scales, T, torch.float32).numpy()
    sc0 = oracle._section(shared["o", 0.0, False][0], lay.scales, T, torch.float32).numpy()
    absmax = np.array([np.abs(g[o:o + n]).max() for o, n in zip(plan.offsets, plan.numels)],
                      dtype=np.float32)
    assert np.array_equal(sc0, absmax)  # clip 0: the largest magnitude
    assert (sc <= absmax).all()
    for t in (0, sim.CONST_T):  # one element, constant: rms = |x|, nothing to clip
        assert sc[t] == absmax[t] > 0
    assert sc[sim.ZERO_T] == 0 and sc0[sim.ZERO_T] == 0
    # the outlier tensor: clip * rms, far below the outlier
    o, n = plan.offsets[sim.OUTLIER_T], plan.numels[sim.OUTLIER_T]
    x = g[o:o + n]
    assert absmax[sim.OUTLIER_T] == sim.OUTLIER
    rms64 = np.sqrt((x.astype(np.float64) ** 2).mean())
    assert sc[sim.OUTLIER_T] == pytest.approx(2.5 * rms64, rel=1e-5)
    assert sc[sim.OUTLIER_T] < 0.1 * sim.OUTLIER
    rms = np.sqrt(np.float32(sim.sumsq(x)) / np.float32(n))
    assert sc[sim.OUTLIER_T] == np.float32(2.5) * rms  # bitwise the fixed-order fp32 definition
    # ... and the outlier itself codes +1 (its probability is capped at 1), decoding to the scaler
    d = oracle.decode_sum(shared["o", 2.5, False][0][None], plan, lay, 1, 1.0).numpy()
    assert d[o + 123] == sc[sim.OUTLIER_T]


def test_sumsq_order_matters_and_matches():
    """The fixed-order sum is the simulation's bit for bit on a multi-chunk tensor, and a tensor of
    more than 256 chunks takes the strided per-thread adds."""
    gen = torch.Generator().manual_seed(5)
    for n in (20000, 257 * 8192 + 3):
        x = torch.randn(n, generator=gen)
        got = np.float32(oracle._tern_sumsq(x))
        if n < 100000:
            assert got == sim.sumsq(x.numpy())
        assert got == pytest.approx(float((x.double() ** 2).sum()), rel=1e-5)


def test_unbiased_without_clipping():
    """The mean of the decoded values over 4096 steps' keys is x to within 5 standard errors of
    the worst element (variance <= scale^2 / 4 per draw).  Deterministic: the RNG is a counter."""
    n, steps = 1024, 4096
    plan = _plan([n], bucket_offset=0)
    lay = Layout.build("tern", plan)
    x = torch.randn(n, generator=torch.Generator().manual_seed(11))
    scale = float(x.abs().max())
    acc = torch.zeros(n, dtype=torch.float64)
    for step in range(steps):
        pay = oracle.encode_tern(x, plan, lay, 0.0, sim.stream_key(0, step, 0))
        acc += oracle.decode_sum(pay[None], plan, lay, 1, 1.0)[:n].double()
    err = float((acc / steps - x.double()).abs().max())
    assert err <= 5 * scale / (2 * np.sqrt(steps)), (err, scale)


@pytest.mark.parametrize("clip", CLIPS)
def test_error_feedback_identity(shared, clip):
    """With x = g + residual_old: residual_new is the one fp32 subtraction x - decoded, bitwise;
    residual_new + decoded == x bitwise wherever that subtraction is exact (a zero code, or
    Sterbenz's |x| / 2 <= |decoded| <= 2 |x| with equal signs) and to the subtraction's half ulp
    elsewhere (fp32 cannot do better: x = 0.01 under decoded = 1 loses its low bits); and what
    clipping removes from the outlier lands in the residual."""
    plan, lay = shared["plan"], shared["lay"]
    pay, res = shared["o", clip, True]
    x = torch.from_numpy(shared["g"]) + torch.from_numpy(shared["r0"])
    d = oracle.decode_sum(pay[None], plan, lay, 1, 1.0)
    own = torch.zeros(plan.length, dtype=torch.bool)
    for o, n in zip(plan.offsets, plan.numels):
        own[o:o + n] = True
    assert torch.equal(res[own].view(torch.int32), (x - d)[own].view(torch.int32))
    exact = own & ((d == 0) | ((x * d > 0) & (d.abs() >= x.abs() / 2) & (d.abs() <= 2 * x.abs())))
    assert exact.sum() > own.sum() // 2 and ((d != 0) & exact).sum() > 100
    assert torch.equal((res + d)[exact].view(torch.int32), x[exact].view(torch.int32))
    x64, d64, r64 = x.double(), d.double(), res.double()
    assert bool(((r64 + d64 - x64).abs() <= 2.0 ** -24 * (x64 - d64).abs())[own].all())
    o = plan.offsets[sim.OUTLIER_T] + 123
    sc = float(oracle._section(pay, lay.scales, plan.num_tensors, torch.float32)[sim.OUTLIER_T])
    assert float(d[o]) == sc
    assert float(res[o]) == float(x[o] - torch.tensor(sc))
    if clip > 0:
        assert float(x[o]) > 50 and float(res[o]) > 0.8 * float(x[o])


def test_payload_size():
    for numels in (sim.NUMELS, [5], [16] * 5, [8192 * 3 + 5, 7, 64, 100003]):
        plan = _plan(numels)
        T, D = len(numels), sum((n + 15) // 16 * 16 for n in numels)
        assert plan.total_codes == D
        lay = Layout.build("tern", plan)
        assert lay.nbytes == _align(_align(4 * T) + D // 4) == sim.layout(numels)[2]
        assert lay.codes == _align(4 * T) and lay.scales == 0 and lay.bits == 2


def test_vgg11_ratio():
    from ewdml.models import build_model
    from ewdml.parallel.flat import FlatModel

    flat = FlatModel(build_model("VGG11"), bucket_bytes=16 << 20)
    c = Codec("tern").bind([b.plan for b in flat.buckets], "cpu")
    sent = sum(c.payload_bytes(i) for i in range(len(flat.buckets)))
    dense = sum(c.dense_bytes(i) for i in range(len(flat.buckets)))
    assert abs(dense / sent - 16) < 0.16, dense / sent


def test_codec_object():
    assert Codec("tern").describe() == "tern2b(c=2.5)"
    assert Codec("tern", clip=3).describe() == "tern2b(c=3)"
    assert Codec("tern", clip=0).describe() == "tern2b"
    with pytest.raises(ValueError, match="belongs to the tern codec"):
        Codec("qsgd", clip=1.0)
    with pytest.raises(ValueError, match=">= 0"):
        Codec("tern", clip=-1.0)
    with pytest.raises(ValueError, match="no encode-side apply"):
        c = Codec("tern").bind([_plan([64])], "cpu")
        c.encode(0, torch.zeros(64), torch.zeros(64, dtype=torch.uint8), 1, 0, apply={})
    got = plan_graph_mode(4, "rccl-stream", "tern", 1 << 20)
    assert got["wire_bytes"] == 3 * (1 << 18)


def test_codec_roundtrip_cpu(shared):
    """The codec object's CPU path is the oracle's, key and clip included."""
    plan, lay = shared["plan"], shared["lay"]
    c = Codec("tern", seed=3).bind([plan], "cpu")
    assert c.layouts[0] == lay and c.key(7, 1) == KEY
    pay = torch.full((lay.nbytes + 32,), 0xFF, dtype=torch.uint8)
    c.encode(0, torch.from_numpy(shared["g"]), pay, 7, 1)
    assert torch.equal(pay[:lay.nbytes], shared["o", 2.5, False][0])
    out = torch.zeros(plan.length)
    c.decode(0, pay[None, :lay.nbytes], out, 1.0)
    assert torch.equal(out, oracle.decode_sum(pay[None, :lay.nbytes], plan, lay, 1, 1.0))


def test_horovod_compression():
    from ewdml.parallel.horovod import Compression

    assert Compression.tern().describe() == "tern2b(c=2.5)"
    assert Compression.tern(clip=0.0).describe() == "tern2b"


def _resolve(*flags):
    return ewdml.parse_args(["--compress", "tern", *flags]).resolved()


def test_cli():
    c = _resolve()
    assert c.tern_clip == 2.5 and c.error_feedback is False
    assert _resolve("--tern-clip", "0").tern_clip == 0.0
    assert _resolve("--tern-clip", "3.5").tern_clip == 3.5
    assert _resolve("--error-feedback").error_feedback is True
    for opt in ("adam", "lars", "lamb"):
        assert _resolve("--optimizer", opt).optimizer == opt
    assert _resolve("--hip-graph", "full").hip_graph == "full"


@pytest.mark.parametrize("flags,reason", [
    (["--topology", "ps"], "--topology ps"),
    (["--topology", "sharded"], "--topology sharded"),
    (["--topology", "twostage"], "--topology twostage"),
    (["--sync-every", "4"], "--sync-every"),
    (["--select-best"], "--select-best"),
    (["--optimizer", "onebit_adam", "--onebit-warmup-steps", "2"], "onebit_adam"),
    (["--optimizer", "onebit_lamb", "--onebit-warmup-steps", "2"], "onebit_lamb"),
    (["--tern-clip", "-1"], "--tern-clip"),
])
def test_cli_refusals(flags, reason):
    with pytest.raises(ValueError, match="--compress tern .*" + reason):
        _resolve(*flags)


def test_cli_refuses_the_clip_elsewhere_and_the_pull():
    with pytest.raises(ValueError, match="--tern-clip belongs to --compress tern"):
        ewdml.parse_args(["--compress", "qsgd", "--tern-clip", "2.5"]).resolved()
    with pytest.raises(SystemExit):  # the pull codecs' choices stay as they were
        ewdml.parse_args(["--topology", "ps", "--pull-compress", "tern"])
    from ewdml.config import Config
    with pytest.raises(ValueError, match="--pull-compress tern"):
        Config(topology="ps", compress="qsgd", pull_compress="tern").resolved()
    with pytest.raises(ValueError, match="--compress tern has no parameter-server form"):
        Config(compress="tern", pull_compress="qsgd").resolved()
