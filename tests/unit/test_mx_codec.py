"""The MXFP8 / MXFP4 oracle (compress/oracle.py mx_*, encode_mx) against the OCP Microscaling v1.0
rules, torch's own E4M3 cast, and the error bounds that 3 and 1 mantissa bits give; the payload
layout's pads; the command line's refusals."""
import pytest
import torch

import ewdml
from ewdml.compress import oracle
from ewdml.compress.codecs import Codec
from ewdml.compress.plan import BucketPlan, Layout
from ewdml.parallel.engine import plan_graph_mode

BITS = [8, 4]
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


def _blocks(x):
    """Pad a flat tensor with zeros to whole blocks: fp32 [B, 32]."""
    x = x.float()
    return torch.cat([x, torch.zeros(-x.numel() % 32)]).reshape(-1, 32)


def _quant_at(x, bits, s=127):
    """Codes of the values ``x`` under a fixed scale byte (X = 1 for 127)."""
    b = _blocks(x)
    return oracle.mx_quantize(b, torch.full((b.shape[0],), s, dtype=torch.int64),
                              bits).flatten()[:x.numel()]


def _values(codes, bits, s=127):
    b = torch.cat([codes, codes.new_zeros(-codes.numel() % 32)]).reshape(-1, 32)
    return oracle.mx_dequantize(b, torch.full((b.shape[0],), s, dtype=torch.int64),
                                bits).flatten()[:codes.numel()]


@pytest.mark.parametrize("bits", BITS)
def test_grid_exhaustive(bits):
    """Every code decodes to the format's value and encodes back to itself (-0 included); E4M3's
    two NaN codes decode to NaN and are never written."""
    codes = torch.arange(1 << bits, dtype=torch.uint8)
    v = _values(codes, bits)
    if bits == 8:
        nan = (codes & 0x7F) == 0x7F
        assert torch.isnan(v[nan]).all() and nan.sum() == 2
        assert torch.equal(v[~nan], codes[~nan].view(torch.float8_e4m3fn).float())
        assert float(v[0x7E]) == 448.0 and float(v[0x01]) == 2.0 ** -9
        codes, v = codes[~nan], v[~nan]
    else:
        assert v.tolist() == [0.0, 0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 6.0,
                              -0.0, -0.5, -1.0, -1.5, -2.0, -3.0, -4.0, -6.0]
    assert torch.equal(_quant_at(v, bits), codes)
    for s in (0, 1, 126, 200, 254 - oracle.MX_FORMATS[bits][4]):  # the scale only shifts
        vs = _values(codes, bits, s)
        assert torch.equal(vs.double(), v.double() * 2.0 ** (s - 127))
        assert torch.equal(_quant_at(vs, bits, s), codes)


@pytest.mark.parametrize("bits", BITS)
def test_ties_go_to_even(bits):
    half = 1 << (bits - 1)
    codes = torch.arange(half - (1 if bits == 8 else 0), dtype=torch.uint8)  # 0 .. largest finite
    v = _values(codes, bits).double()
    for s in (127, 0, 240):
        X = 2.0 ** (s - 127)
        mid = (((v[:-1] + v[1:]) / 2) * X).float()
        assert torch.equal(mid.double(), (v[:-1] + v[1:]) / 2 * X)  # representable: a true tie
        even = torch.where(codes[:-1] % 2 == 0, codes[:-1], codes[1:])
        below = (mid.view(torch.int32) - 1).view(torch.float32)
        above = (mid.view(torch.int32) + 1).view(torch.float32)
        for sign, bit in ((1.0, 0), (-1.0, half)):
            assert torch.equal(_quant_at(sign * mid, bits, s), even | bit)
            assert torch.equal(_quant_at(sign * below, bits, s), codes[:-1] | bit)
            assert torch.equal(_quant_at(sign * above, bits, s), codes[1:] | bit)


def test_e4m3_rounding_is_torchs():
    """An independent check: for |q| <= 448 torch's float8_e4m3fn cast rounds the same way; beyond
    it torch gives NaN where this codec saturates."""
    gen = torch.Generator().manual_seed(0)
    q = torch.cat([torch.randn(1 << 16, generator=gen) * 40,
                   torch.randn(1 << 14, generator=gen) * 0.01,
                   torch.linspace(-448, 448, 4097), torch.tensor([0.0, -0.0, 2.0 ** -10, 1e-9])])
    q = q.clamp(-448, 448)
    assert torch.equal(_quant_at(q, 8), q.to(torch.float8_e4m3fn).view(torch.uint8))
    over = torch.tensor([448.1, 464.0, 480.0, 511.0, -500.0])
    assert _quant_at(over, 8).tolist() == [0x7E, 0x7E, 0x7E, 0x7E, 0xFE]
    assert _quant_at(torch.tensor([6.1, 7.0, 7.99, -7.5]), 4).tolist() == [0x7, 0x7, 0x7, 0xF]


@pytest.mark.parametrize("bits", BITS)
def test_scale_rule(bits):
    """s = clamp(em - emax, 0, 254) for every exponent field of the block's largest element, from
    zeros and denormals (em = 0) to 254; 0xFF where the block holds an inf or a NaN."""
    emax = oracle.MX_FORMATS[bits][4]
    em = torch.arange(255, dtype=torch.int32)
    big = ((em << 23) | 0x2AAAAA).view(torch.float32)  # any mantissa: only the field counts
    blocks = torch.zeros(255, 32)
    blocks[:, 5] = -big
    blocks[1:, 9] = ((em[1:] - 1) << 23 | 0x7FFFFF).view(torch.float32)  # smaller exponents lose
    s = oracle.mx_scale_bytes(blocks, bits)
    assert torch.equal(s, (em.long() - emax).clamp(0, 254))
    assert int(oracle.mx_scale_bytes(torch.zeros(1, 32), bits)) == 0
    bad = torch.ones(3, 32)
    bad[0, 31], bad[1, 0], bad[2, 3] = float("inf"), float("nan"), -float("inf")
    assert oracle.mx_scale_bytes(bad, bits).tolist() == [255, 255, 255]
    # a NaN with a small payload is not dropped by the maximum, nor is a negative one
    nan = torch.tensor([0x7F800001, 0xFFC00000 - (1 << 32)], dtype=torch.int64).to(torch.int32)
    bad = torch.ones(2, 32) * 3e38
    bad[0, 1], bad[1, 2] = nan.view(torch.float32)[0], nan.view(torch.float32)[1]
    assert oracle.mx_scale_bytes(bad, bits).tolist() == [255, 255]
    codes = oracle.mx_quantize(bad, torch.tensor([255, 255]), bits)
    assert not codes.any()
    assert torch.isnan(oracle.mx_dequantize(codes, torch.tensor([255, 255]), bits)).all()


@pytest.mark.parametrize("bits", BITS)
def test_error_bounds(bits):
    """Per element: E4M3 |e - d| <= max(|e| 2^-4, X 2^-10), or < 64 X where saturated; E2M1 |e - d|
    <= max(|e| 2^-2, X / 4), or < 2 X where saturated."""
    _, mb, _, top, _ = oracle.MX_FORMATS[bits]
    gen = torch.Generator().manual_seed(1)
    e = torch.randn(4096, 32, generator=gen) * torch.exp(torch.randn(4096, 1, generator=gen) * 8)
    e[::7, 3] *= 1.9  # more blocks whose largest element lands in the saturation band
    s = oracle.mx_scale_bytes(e, bits)
    codes = oracle.mx_quantize(e, s, bits)
    d = oracle.mx_dequantize(codes, s, bits).double()
    X = (2.0 ** (s.double() - 127))[:, None].expand_as(d)
    err, mag = (e.double() - d).abs(), e.double().abs()
    sat = mag > top * X
    assert sat.any() and ((codes & ((1 << (bits - 1)) - 1))[sat] == (0x7E if bits == 8 else 7)).all()
    assert (err[sat] < (64 if bits == 8 else 2) * X[sat]).all()
    rel, floor = 2.0 ** -(mb + 1), (2.0 ** -10 if bits == 8 else 0.25)
    assert (err[~sat] <= torch.maximum(mag[~sat] * rel, X[~sat] * floor)).all()
    # the residual is that difference, one fp32 subtract
    plan = _plan([e.numel()])
    lay = Layout.build("mx", plan, bits)
    r = torch.zeros(plan.length)
    pay = oracle.encode_mx(e.flatten(), plan, lay, r)
    assert torch.equal(r, e.flatten() - d.float().flatten())
    assert torch.equal(oracle.decode_sum(pay[None], plan, lay, 0, 1.0), d.float().flatten())


@pytest.mark.parametrize("bits", BITS)
@pytest.mark.parametrize("numels", SHAPES)
def test_layout_bytes_and_pads(numels, bits):
    plan = _plan(numels)
    lay = Layout.build("mx", plan, bits)
    L = plan.length
    assert lay.scales == 0 and lay.codes == (L // 32 + 15) // 16 * 16
    assert lay.nbytes == lay.codes + L * bits // 8 and lay.nbytes % 16 == 0
    g = _grad(plan, seed=3)
    g[g == 0] = 1.0  # the pads hold garbage the encode must not send
    pay = oracle.encode_mx(g, plan, lay)
    own = torch.zeros(L, dtype=torch.bool)
    for off, n in zip(plan.offsets, plan.numels):
        own[off:off + n] = True
    codes = pay[lay.codes:lay.codes + L * bits // 8]
    if bits == 4:
        codes = torch.stack([codes & 0xF, codes >> 4], 1).flatten()
    assert not codes[~own].any() and codes[own].any()
    assert not pay[L // 32:lay.codes].any()  # the alignment pad
    blocks_own = own.reshape(-1, 32).any(1)
    assert not pay[:L // 32][~blocks_own].any()  # a block of pad positions only: scale byte 0
    # decode: element i is code i under scale byte i >> 5, the pads stay 0
    d = oracle.decode_sum(pay[None], plan, lay, 0, 1.0)
    s = pay[:L // 32].long()
    want = oracle.mx_dequantize(codes.reshape(-1, 32), s, bits).flatten()
    assert torch.equal(d[own], want[own]) and not d[~own].any()


def test_layout_needs_packed_tensors():
    with pytest.raises(ValueError):
        Layout.build("mx", BucketPlan([100, 100], [0, 100]), 8)
    with pytest.raises(ValueError):
        Layout.build("mx", BucketPlan([100, 100], [0, 256], 1.0, 0, 384), 8)
    with pytest.raises(ValueError):
        Layout.build("mx", _plan([100]), 6)


def test_nonfinite_block_decodes_to_nan_everywhere():
    plan = _plan([96, 40])
    g = _grad(plan, seed=2)
    g[40] = float("inf")
    g[plan.offsets[1] + 39] = float("nan")
    for bits in BITS:
        lay = Layout.build("mx", plan, bits)
        r = torch.zeros(plan.length)
        pay = oracle.encode_mx(g, plan, lay, r)
        sb = pay[:plan.length // 32].tolist()  # blocks 0..2: tensor 0, 3: its pad, 4..5: tensor 1
        assert sb[1] == 255 and sb[3] == 0 and sb[5] == 255 and 0 < min(sb[0], sb[2], sb[4]) < 255
        d = oracle.decode_sum(torch.stack([pay, pay]), plan, lay, 0, 0.5)
        assert torch.isnan(d[32:64]).all() and torch.isfinite(d[:32]).all()
        assert torch.isnan(r[32:64]).all() and torch.isfinite(r[64:96]).all()
        o = plan.offsets[1]
        assert torch.isnan(d[o + 32:o + 40]).all() and not d[o + 40:].any()  # pads stay 0
        assert torch.isnan(r[o + 32:o + 40]).all() and not r[o + 40:].any()


def test_describe_and_wire_size():
    assert Codec("mx").describe() == "mxfp8" and Codec("mx", fmt="fp4").describe() == "mxfp4"
    with pytest.raises(ValueError):
        Codec("mx", fmt="fp6")
    with pytest.raises(ValueError):
        Codec("sign", fmt="fp8")
    plan = _plan([1 << 20])
    for fmt, per in (("fp8", 33 / 32), ("fp4", 17 / 32)):
        c = Codec("mx", fmt=fmt).bind([plan], "cpu")
        assert c.payload_bytes(0) == int(per * (1 << 20))
        got = plan_graph_mode(4, "rccl-stream", "mx", 1 << 20, bits=c.bits)
        assert got["wire_bytes"] == 3 * int(per * (1 << 20))


def test_horovod_compression():
    from ewdml.parallel.horovod import Compression

    assert Compression.mx().describe() == "mxfp8"
    assert Compression.mx(fmt="fp4").describe() == "mxfp4"


def _resolve(*flags):
    return ewdml.parse_args(["--compress", "mx", *flags]).resolved()


def test_cli():
    c = _resolve()
    assert c.mx_format == "fp8" and c.error_feedback is True
    assert _resolve("--mx-format", "fp4").mx_format == "fp4"
    assert _resolve("--no-error-feedback").error_feedback is False
    for opt in ("adam", "lars", "lamb", "lion"):
        assert _resolve("--optimizer", opt).optimizer == opt
    assert _resolve("--clip-grad-norm", "1.0").clip_grad_norm == 1.0


@pytest.mark.parametrize("flags,reason", [
    (["--topology", "ps"], "--topology ps"),
    (["--topology", "sharded"], "--topology sharded"),
    (["--topology", "twostage"], "--topology twostage"),
    (["--sync-every", "4"], "--sync-every"),
    (["--select-best"], "--select-best"),
    (["--optimizer", "onebit_adam", "--onebit-warmup-steps", "2"], "onebit_adam"),
    (["--optimizer", "onebit_lamb", "--onebit-warmup-steps", "2"], "onebit_lamb"),
    (["--vote-aggregate", "average"], "--compress vote"),
    (["--vote-exchange", "twostage"], "--compress vote"),
    (["--sign-rotate", "hadamard"], "--compress sign"),
])
def test_cli_refusals(flags, reason):
    with pytest.raises(ValueError, match=reason):
        _resolve(*flags)


def test_cli_refuses_the_format_elsewhere_and_the_pull():
    with pytest.raises(ValueError, match="--mx-format belongs to --compress mx"):
        ewdml.parse_args(["--compress", "sign", "--mx-format", "fp4"]).resolved()
    with pytest.raises(SystemExit):  # the pull codecs' choices stay as they were
        ewdml.parse_args(["--topology", "ps", "--pull-compress", "mx"])
    with pytest.raises(SystemExit):
        ewdml.parse_args(["--compress", "mx", "--mx-format", "fp6"])
    from ewdml.config import Config
    with pytest.raises(ValueError, match="--pull-compress mx"):
        Config(topology="ps", compress="qsgd", pull_compress="mx").resolved()
