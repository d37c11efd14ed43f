"""The 1-bit sign codec on the CPU: payload layout, the torch oracle (compress/oracle.py
encode_sign / decode_sum), error-feedback telescoping, and the CLI / config / API plumbing."""
import numpy as np
import pytest
import torch

import ewdml
from ewdml.compress import Codec, oracle
from ewdml.compress.plan import CHUNK, BucketPlan, Layout

PLANS = [[10], [500, 10], [8192 * 3 + 5, 7, 64, 100003]]


def _plan(numels, bucket_offset=0):
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


def _chunks(plan):
    return list(zip(plan.chunk_start, plan.chunk_len))


def _unpack(pay, plan, lay):
    """(scales [C], bits [C, CHUNK] bool) of a payload, read independently of the oracle."""
    C = plan.num_chunks
    raw = pay.numpy()
    scales = raw[lay.scales:lay.scales + 4 * C].view(np.float32)
    words = raw[lay.codes:lay.codes + 1024 * C].view(np.uint32).reshape(C, CHUNK // 32)
    bits = (words[:, :, None] >> np.arange(32, dtype=np.uint32)) & 1
    return scales, bits.reshape(C, CHUNK).astype(bool)


@pytest.mark.parametrize("numels", PLANS)
def test_layout(numels):
    plan = _plan(numels)
    C = plan.num_chunks
    assert C == sum((n + CHUNK - 1) // CHUNK for n in numels)
    lay = Layout.build("sign", plan)
    a16 = (4 * C + 15) // 16 * 16
    assert lay.kind == "sign" and lay.scales == 0 and lay.codes == a16
    assert lay.codes % 16 == 0 and lay.nbytes == a16 + 1024 * C and lay.nbytes % 16 == 0


@pytest.mark.parametrize("ef", [False, True])
@pytest.mark.parametrize("numels", PLANS)
def test_oracle_encode(numels, ef):
    plan = _plan(numels, bucket_offset=4096)
    lay = Layout.build("sign", plan)
    g = _grad(plan, seed=1)
    r0 = _grad(plan, seed=2) * 0.3 if ef else None
    resid = r0.clone() if ef else None
    pay = oracle.encode_sign(g.clone(), plan, lay, resid)
    assert pay.dtype == torch.uint8 and pay.numel() == lay.nbytes
    e = g + r0 if ef else g
    scales, bits = _unpack(pay, plan, lay)
    for c, (s, n) in enumerate(_chunks(plan)):
        x = e[s:s + n]
        assert np.array_equal(bits[c, :n], (x < 0).numpy())
        assert not bits[c, n:].any(), "padding bits must be zero"
        mean = float(x.double().abs().mean())
        assert abs(float(scales[c]) - mean) <= 1e-5 * mean
        if ef:
            d = torch.where(x < 0, -torch.tensor(scales[c]), torch.tensor(scales[c]))
            assert torch.equal(resid[s:s + n], x - d)
    if ef:  # alignment gaps between the tensors are not touched
        keep = torch.ones(plan.length, dtype=torch.bool)
        for off, n in zip(plan.offsets, plan.numels):
            keep[off:off + n] = False
        assert torch.equal(resid[keep], r0[keep])


def test_oracle_zero_and_negative_zero():
    plan = _plan([100, 300])
    lay = Layout.build("sign", plan)
    resid = torch.zeros(plan.length)
    pay = oracle.encode_sign(torch.zeros(plan.length), plan, lay, resid)
    assert not pay.any() and not resid.any()  # scale 0, bits 0, residual stays 0
    g = torch.zeros(plan.length)
    g[0], g[1], g[2], g[3] = -0.0, float("nan"), -1.0, 2.0
    pay = oracle.encode_sign(g, plan, lay)
    _, bits = _unpack(pay, plan, lay)
    assert bits[0, :4].tolist() == [False, False, True, False]  # -0 and NaN give 0


def test_oracle_sum_order_is_the_written_one():
    """_sign_chunk_sums against a scalar transcription of the kernel's order."""
    f32 = np.float32
    gen = torch.Generator().manual_seed(5)
    a = torch.rand(2, CHUNK, generator=gen)
    a[1, 5000:] = 0.0
    got = oracle._sign_chunk_sums(a).numpy()
    for c in range(2):
        x = a[c].numpy()
        th = []
        for t in range(256):
            s = f32(0.0)
            for u in range(8):
                for j in range(4):
                    s = f32(s + x[u * 1024 + 4 * t + j])
            th.append(s)
        tot = f32(0.0)
        for w in range(4):
            v = list(th[64 * w:64 * w + 64])
            d = 32
            while d:
                for i in range(d):
                    v[i] = f32(v[i] + v[i + d])
                d >>= 1
            tot = f32(tot + v[0])
        assert got[c] == tot


def test_oracle_decode_sum_rank_order():
    plan = _plan([8192 + 77, 33], bucket_offset=64)
    lay = Layout.build("sign", plan)
    N = 3
    pays = [oracle.encode_sign(_grad(plan, seed=10 + r) * (10.0 ** r), plan, lay) for r in range(N)]
    recv = torch.stack(pays)
    got = oracle.decode_sum(recv, plan, lay, 127, 1.0 / N)
    acc = torch.zeros(plan.length)
    for r in range(N):  # start from 0, every add rounded, rank order
        scales, bits = _unpack(pays[r], plan, lay)
        for c, (s, n) in enumerate(_chunks(plan)):
            sc = torch.tensor(scales[c])
            acc[s:s + n] = acc[s:s + n] + torch.where(torch.from_numpy(bits[c, :n]), -sc, sc)
    assert torch.equal(got, acc * torch.tensor(1.0 / N, dtype=torch.float32))


def test_error_feedback_telescopes():
    """sum_t decoded_t = T g + r_0 - r_T: the mean decoded vector approaches g at rate 1 / T."""
    plan = _plan([3000, 8192 + 5])
    lay = Layout.build("sign", plan)
    g = _grad(plan, seed=3)
    resid = torch.zeros(plan.length)
    T = 200
    tot = torch.zeros(plan.length, dtype=torch.float64)
    for _ in range(T):
        pay = oracle.encode_sign(g, plan, lay, resid)
        tot += oracle.decode_sum(pay[None], plan, lay, 127, 1.0).double()
    err = (tot / T - g.double()).abs().max()
    assert float(err) <= float(resid.abs().max()) / T + 1e-5


def test_codec_cpu_roundtrip_and_errors():
    plan = _plan([500, 10])
    c = Codec("sign", bits=3, levels=100000).bind([plan], "cpu")  # bits / levels are ignored
    assert c.describe() == "sign1b" and not c.allreduce
    lay = c.layouts[0]
    assert lay.kind == "sign" and c.payload_bytes(0) == lay.nbytes
    g = _grad(plan, seed=4)
    pay = torch.zeros(lay.nbytes, dtype=torch.uint8)
    resid = torch.zeros(plan.length)
    c.encode(0, g, pay, step=3, rank=1, resid=resid)
    assert torch.equal(pay, oracle.encode_sign(g, plan, lay))
    c2 = Codec("sign").bind([plan], "cpu")
    pay2 = torch.zeros_like(pay)
    c2.encode(0, g, pay2, step=9, rank=0)  # no key, step or rank enters the payload
    assert torch.equal(pay, pay2)
    out = torch.zeros(plan.length)
    c.decode(0, pay[None], out, 0.5)
    assert torch.equal(out, oracle.decode_sum(pay[None], plan, lay, 127, 0.5))
    with pytest.raises(ValueError):
        c.encode(0, g, pay, 0, 0, resid=resid, dgc=dict(velocity=resid, momentum=0.9))
    with pytest.raises(ValueError):
        c.encode(0, g, pay, 0, 0, resid=resid, ef21=True)
    with pytest.raises(ValueError):
        c.encode(0, g, pay, 0, 0, apply=dict(param=g))
    with pytest.raises(ValueError):
        c.set_ratio(0.5)


def test_cli_and_config():
    cfg = ewdml.parse_args(["--compress", "sign", "--device", "cpu"])
    assert cfg.compress == "sign" and cfg.error_feedback is True
    assert cfg.topk_warmup == "" and cfg.lr_warmup_epochs == 0  # the warm-up recipe is top-k's
    off = ewdml.parse_args(["--compress", "sign", "--no-error-feedback", "--device", "cpu"])
    assert off.error_feedback is False
    for bad in (["--topology", "ps"], ["--topology", "sharded"], ["--sync-every", "5"]):
        with pytest.raises(ValueError, match="sign"):
            ewdml.parse_args(["--compress", "sign", "--device", "cpu"] + bad)
    # --pull-compress keeps its choices
    with pytest.raises(SystemExit):
        ewdml.parse_args(["--pull-compress", "sign"])


def test_exchange_ef_mode_plain():
    from ewdml.models import build_model
    from ewdml.optim import make_optimizer
    from ewdml.parallel.comm import Comm
    from ewdml.parallel.engine import GradientExchange
    from ewdml.parallel.flat import FlatModel

    flat = FlatModel(build_model("LeNet"), bucket_bytes=16 << 20)
    opt = make_optimizer("sgd", flat, lr=0.01, momentum=0.9)
    ex = GradientExchange(flat, Comm(), Codec("sign"), opt, overlap=False,
                          error_feedback=True, ef_mode="dgc")
    assert ex.ef_mode == "plain" and ex.resid is not None and ex.vel is None
    assert ex.enable_local_apply() is False
    assert ex.codec_health() == {}
    ex.close()


def test_horovod_compression_sign():
    from ewdml.parallel.horovod import Compression

    c = Compression.sign()
    assert isinstance(c, Codec) and c.kind == "sign"


@pytest.mark.parametrize("world", [2, 8])
def test_plan_graph_mode_wire_bytes(world):
    from ewdml.parallel.engine import plan_graph_mode

    numel = 9_231_114
    out = plan_graph_mode(world, "rccl-stream", "sign", numel)
    assert out["wire_bytes"] == int((world - 1) * numel / 8)
