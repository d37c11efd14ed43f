"""The gradient clip's two gfx950 launches (``ops/csrc/clip.hip``: k_clip_norm, k_clip_scale) on
one MI355X against a float64 reference.

One model of seven 1-D tensors -- 1, 63, 64, 8191, 8192, 8193 and 3 * 8192 + 5 elements: below a
chunk, one chunk less / exactly / plus one element, four chunks with a 1-element scalar tail --
laid out once as one bucket and once as two.  The gradients come once as the flat fp32 view
(NaN-bit sentinels in the alignment padding) and once as a pointer-mode list of separate tensors
with fp32 and bf16 mixed.

Bound.  With u = 2^-24: a chunk's partial is a sum of non-negative squares, each rounded once
(u), through a chain of at most L = ``ops.CLIP_SUM_CHAIN`` fp32 additions, so it is off by at most
(L + 1) u relative; the fp64 total over the partials adds nothing at this scale and keeps that
relative bound.  The square root halves it and its rounding to fp32 adds u: ``norm`` is within
((L + 1) / 2 + 1) u <= (L + 2) u of the float64 norm.  ``coef = C / (norm + 1e-6f)`` adds the
rounding of the sum and of the quotient: ((L + 1) / 2 + 3) u <= (L + 2) u for L >= 3.  The
reference uses the fp32 value of C that the kernel receives.
"""
import functools
import struct

import pytest
import torch

from ewdml import ops
from ewdml.parallel.clip import GradClipper
from ewdml.parallel.flat import FlatModel

pytestmark = pytest.mark.gpu

DEV = "cuda"
SIZES = [1, 63, 64, 8191, 8192, 8193, 3 * 8192 + 5]
BF16 = (1, 3, 5)  # pointer mode: these tensors are bf16
SPLIT_BYTES = 40000  # [1 .. 8192] | [8193, 3 * 8192 + 5]
SENTINEL = 0x7FC12345  # a NaN's bits
C_ACTIVE = 3.0


def _f32(x):
    return struct.unpack("f", struct.pack("f", x))[0]


@functools.lru_cache(maxsize=None)
def _values(zero=False):
    """The gradient values, made once on the CPU and left unchanged."""
    g = torch.Generator().manual_seed(11)
    return tuple(torch.zeros(n) if zero else torch.randn(n, generator=g) * (0.5 + i)
                 for i, n in enumerate(SIZES))


def _model(split, attach):
    ps = [torch.nn.Parameter(torch.zeros(n, device=DEV)) for n in SIZES]
    flat = FlatModel(ps, bucket_bytes=SPLIT_BYTES if split else 1 << 30, reverse=False,
                     attach_grads=attach)
    assert len(flat.buckets) == (2 if split else 1)
    return flat


def _fill(flat, mode, zero=False):
    """The per-tensor gradient tensors (views of the flat buffer, or separate ones) and what
    each bucket's launch takes."""
    vals = _values(zero)
    if mode == "flat":
        flat.grad.view(torch.int32).fill_(SENTINEL)
        ts = []
        for p, o, v in zip(flat.params, flat.offsets, vals):
            flat.grad[o:o + p.numel()].copy_(v)
            ts.append(flat.grad[o:o + p.numel()])
        return ts, [flat.grad_view(b) for b in flat.buckets]
    ts = [(v.bfloat16() if i in BF16 else v).to(DEV) for i, v in enumerate(vals)]
    per, i = [], 0
    for b in flat.buckets:
        per.append(ts[i:i + len(b.params)])
        i += len(b.params)
    return ts, per


def _clip(split, mode, C, zero=False):
    flat = _model(split, attach=mode == "flat")
    ts, per = _fill(flat, mode, zero)
    before = [t.clone() for t in ts]
    whole = flat.grad.clone()
    cp = ops.ClipPlan([b.plan for b in flat.buckets], DEV)
    assert cp.total_chunks == sum((n + 8191) // 8192 for n in SIZES) == cp.partials.numel()
    for b, g in zip(flat.buckets, per):
        ops.clip_norm(cp, b.index, g)
    for b, g in zip(flat.buckets, per):
        ops.clip_scale(cp, b.index, g, C)
    torch.cuda.synchronize()
    return dict(flat=flat, ts=ts, before=before, whole=whole, state=cp.state.clone(),
                partials=cp.partials.clone())


@functools.lru_cache(maxsize=None)
def _norm64(mode):
    vals = [(v.bfloat16() if (mode == "ptr" and i in BF16) else v).double()
            for i, v in enumerate(_values())]
    return float(torch.sqrt(sum((v * v).sum() for v in vals)))


def _bits(t):
    return t.contiguous().view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32)


@pytest.mark.parametrize("split", [False, True], ids=["one_bucket", "two_buckets"])
@pytest.mark.parametrize("mode", ["flat", "ptr"])
def test_active_clip(mode, split):
    ops.require()
    r = _clip(split, mode, C_ACTIVE)
    norm, coef = (float(v) for v in r["state"])
    ref = _norm64(mode)
    ref_coef = _f32(C_ACTIVE) / (ref + 1e-6)
    bound = (ops.CLIP_SUM_CHAIN + 2) * 2.0 ** -24
    print(f"{mode} split={split}: norm {norm!r} ref {ref!r} rel {abs(norm - ref) / ref:.3e}; "
          f"coef {coef!r} ref {ref_coef!r} rel {abs(coef - ref_coef) / ref_coef:.3e} "
          f"(bound {bound:.3e})")
    assert ops.CLIP_SUM_CHAIN == 41
    assert abs(norm - ref) <= bound * ref
    assert coef < 1.0 and abs(coef - ref_coef) <= bound * ref_coef
    # the scaled gradient: bitwise g * coef_dev, one fp32 multiply (bf16: rounded to nearest even)
    coef_dev = r["state"][1]
    for i, (got, b) in enumerate(zip(r["ts"], r["before"])):
        want = (b.float() * coef_dev).bfloat16() if b.dtype == torch.bfloat16 else b * coef_dev
        assert got.dtype == b.dtype and torch.equal(_bits(got), _bits(want)), SIZES[i]
        assert not torch.equal(_bits(got), _bits(b))
    if mode == "flat":  # the padding between the tensors: neither read (finite norm) nor written
        flat = r["flat"]
        pad = torch.ones(flat.numel, dtype=torch.bool, device=DEV)
        for p, o in zip(flat.params, flat.offsets):
            pad[o:o + p.numel()] = False
        assert int(pad.sum()) > 0 and norm == norm and norm != float("inf")
        assert bool((flat.grad.view(torch.int32)[pad] == SENTINEL).all())


@pytest.mark.parametrize("mode", ["flat", "ptr"])
def test_inactive_clip_touches_nothing(mode):
    ops.require()
    r = _clip(True, mode, 1e9)
    ref = _norm64(mode)
    assert float(r["state"][1]) == 1.0
    assert abs(float(r["state"][0]) - ref) <= (ops.CLIP_SUM_CHAIN + 2) * 2.0 ** -24 * ref
    for got, b in zip(r["ts"], r["before"]):
        assert torch.equal(_bits(got), _bits(b))
    if mode == "flat":
        assert torch.equal(r["flat"].grad.view(torch.int32), r["whole"].view(torch.int32))


@pytest.mark.parametrize("mode", ["flat", "ptr"])
def test_zero_gradient(mode):
    ops.require()
    r = _clip(True, mode, 0.5, zero=True)
    assert r["state"].tolist() == [0.0, 1.0]
    assert all(bool((t.float() == 0).all()) for t in r["ts"])


@pytest.mark.parametrize("mode", ["flat", "ptr"])
def test_bitwise_reproducible_and_independent_of_the_bucket_cut(mode):
    ops.require()
    a, b, one = _clip(True, mode, C_ACTIVE), _clip(True, mode, C_ACTIVE), \
        _clip(False, mode, C_ACTIVE)
    for other in (b, one):
        assert torch.equal(_bits(a["state"]), _bits(other["state"]))
        assert torch.equal(_bits(a["partials"]), _bits(other["partials"]))  # chunk order
        for x, y in zip(a["ts"], other["ts"]):
            assert torch.equal(_bits(x), _bits(y))


def test_clipper_runs_the_same_launches():
    ops.require()
    flat = _model(True, attach=True)
    ts, _ = _fill(flat, "flat")
    clip = GradClipper(flat, 4 * C_ACTIVE, world=16, scale_world=True)  # C / sqrt(16)
    assert clip.max_norm == C_ACTIVE and clip.last() is None
    clip.run()
    want = _clip(True, "flat", C_ACTIVE)
    assert torch.equal(_bits(clip.plan.state), _bits(want["state"]))
    assert clip.last() == tuple(want["state"].tolist())
    assert torch.equal(flat.grad.view(torch.int32), want["flat"].grad.view(torch.int32))


def test_argument_checks():
    ops.require()
    flat = _model(True, attach=True)
    _, per = _fill(flat, "flat")
    cp = ops.ClipPlan([b.plan for b in flat.buckets], DEV)
    with pytest.raises(ValueError, match="max_norm must be > 0"):
        ops.clip_scale(cp, 0, per[0], 0.0)
    with pytest.raises(ValueError, match="bucket 2 of a clip plan of 2"):
        ops.clip_norm(cp, 2, per[0])
    with pytest.raises(ValueError, match="must be a device tensor"):
        ops.clip_norm(cp, 0, per[0].cpu())
    with pytest.raises(ValueError, match="bucket needs"):
        ops.clip_norm(cp, 0, per[0][:64])
    with pytest.raises(ValueError, match="gradients for a bucket of"):
        ops.clip_norm(cp, 0, [per[0]])
    with pytest.raises(TypeError, match="expected torch.float32"):
        ops.clip_norm(cp, 0, per[0].half())
    with pytest.raises(ValueError, match="needs a GPU device"):
        ops.ClipPlan([b.plan for b in flat.buckets], "cpu")
