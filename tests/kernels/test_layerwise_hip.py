"""The layer-wise optimizers' two gfx950 launches (``ops/csrc/layerwise.hip``: k_lw_stage,
k_lw_apply) through ``FlatLARS`` / ``FlatLAMB`` on one MI355X, against the torch oracle on the CPU
and a float64 reference.

One flat model: a 1-D tensor, a small matrix, exactly one chunk, a chunk plus one element, five
rows of 4000 and ``[1, 16385]`` (three chunks, a 1-element scalar tail), split so that the whole
model spans two buckets.  Three steps.  Parameters and state are checked at the project's Adam
tolerance; the trust ratios against float64 within ``2 (L + 2) 2^-24`` relative: each norm's sum
of non-negative terms through a chain of L fp32 additions is off by at most ``(L + 2) 2^-24``,
the square root halves that and the ratio adds two of them (L = ``ops.LAYERWISE_SUM_CHAIN``).
"""
import functools

import pytest
import torch

from ewdml import ops
from tests.layerwise_ref import SHAPES, Ref64, make_flat, make_grad, split

pytestmark = pytest.mark.gpu

DEV = "cuda"
SHAPES6 = SHAPES + [(1, 16385)]
BUCKET_BYTES = 104000  # the first five tensors | [1, 16385]
STEPS = 3
# case -> hyper-parameters; the rule is the case's first word.  The *_plain / *_nesterov / *_nowd
# cases take the kernels' other branches: no momentum state, Nesterov, weight decay 0
KW = {"lars": dict(lr=0.1, momentum=0.9, dampening=0.1, weight_decay=1e-2, eta=0.01),
      "lamb": dict(lr=0.01, weight_decay=1e-2),
      "lars_plain": dict(lr=0.1, eta=0.01),
      "lars_nesterov": dict(lr=0.1, momentum=0.9, nesterov=True, eta=0.01),
      "lamb_nowd": dict(lr=0.01)}
DTYPES = {"fp32": torch.float32, "bf16": torch.bfloat16, "fp16": torch.float16}


def _opt(kind, flat):
    from ewdml.optim import FlatLAMB, FlatLARS

    return (FlatLARS if kind.startswith("lars") else FlatLAMB)(flat, **KW[kind])


def _state(flat, opt):
    out = {"p": flat.data}
    if opt.kind == "lamb":
        out.update(exp_avg=opt.exp_avg, exp_avg_sq=opt.exp_avg_sq)
    else:
        out["mom"] = opt.mom
    return {k: v.detach().cpu().clone() for k, v in out.items()}


def _run(device, kind, gdt, grad_scale, per_bucket=False, shadow=False):
    """Three steps; the state after the last and the ratios of every step."""
    flat = make_flat(SHAPES6, device=device, bucket_bytes=BUCKET_BYTES)
    assert len(flat.buckets) == 2
    if shadow:
        flat.shadow = torch.zeros(flat.numel, dtype=torch.bfloat16, device=device)
    opt = _opt(kind, flat)
    ratios = []
    for s in range(STEPS):
        g = make_grad(flat, s, DTYPES[gdt])
        if per_bucket:
            for b in flat.buckets:
                opt.step_range(b.start, b.length, g[b.start:b.start + b.length], grad_scale)
            opt.end_step()
        else:
            opt.step(grad=g, grad_scale=grad_scale)
        ratios.append(opt.ratio.detach().cpu().clone())
    st = _state(flat, opt)
    st["ratios"] = ratios
    st["shadow"] = flat.shadow.cpu() if shadow else None
    return st


@functools.lru_cache(maxsize=None)
def _oracle(kind, gdt, grad_scale):
    """The torch oracle on the CPU (computed once per case and shared)."""
    return _run("cpu", kind, gdt, grad_scale)


@functools.lru_cache(maxsize=None)
def _ratios64(kind, gdt, grad_scale):
    flat = make_flat(SHAPES6, bucket_bytes=BUCKET_BYTES)
    kw = dict(KW[kind])
    ref = Ref64(kind.split("_")[0], flat, kw.pop("lr"), kw.pop("weight_decay", 0.0), **kw)
    out = []
    for s in range(STEPS):
        ref.step(split(flat, make_grad(flat, s, DTYPES[gdt])), grad_scale)
        out.append(torch.tensor(ref.ratios, dtype=torch.float64))
    return out


def _bits(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32),
                                              b.contiguous().view(torch.int32))


CASES = [("fp32", 1.0), ("bf16", 0.5), ("fp16", 0.5)]


@pytest.mark.parametrize("gdt,grad_scale", CASES)
@pytest.mark.parametrize("kind", ["lars", "lamb"])
def test_three_steps_match_the_oracle(kind, gdt, grad_scale):
    ops.require()
    want = _oracle(kind, gdt, grad_scale)
    whole = _run(DEV, kind, gdt, grad_scale)
    for k in ("p", "exp_avg", "exp_avg_sq", "mom"):
        if k in want:
            torch.testing.assert_close(whole[k], want[k], rtol=1e-5, atol=1e-6, msg=k)
    assert not _bits(whole["p"], make_flat(SHAPES6, bucket_bytes=BUCKET_BYTES).data)
    # trust ratios against float64
    bound = 2 * (ops.LAYERWISE_SUM_CHAIN + 2) * 2.0 ** -24
    for s, (got, ref) in enumerate(zip(whole["ratios"], _ratios64(kind, gdt, grad_scale))):
        rel = ((got.double() - ref) / ref).abs()
        print(f"{kind} {gdt} step {s + 1}: ratio rel err max {float(rel.max()):.3e} "
              f"(bound {bound:.3e})")
        assert float(rel.max()) <= bound, (s, rel)
        assert float(got[0]) == 1.0 and bool((got[1:] != 1.0).all())
    _check_bitwise_and_padding(kind, gdt, grad_scale, whole)


@pytest.mark.parametrize("kind", ["lars_plain", "lars_nesterov", "lamb_nowd"])
def test_other_branches_match_the_oracle(kind):
    """No momentum (the buffer is neither read nor written), Nesterov, and weight decay 0."""
    ops.require()
    want = _oracle(kind, "fp32", 0.5)
    whole = _run(DEV, kind, "fp32", 0.5)
    for k in ("p", "exp_avg", "exp_avg_sq", "mom"):
        if k in want:
            torch.testing.assert_close(whole[k], want[k], rtol=1e-5, atol=1e-6, msg=k)
    if kind == "lars_plain":
        assert not bool(whole["mom"].any())
    bound = 2 * (ops.LAYERWISE_SUM_CHAIN + 2) * 2.0 ** -24
    for got, ref in zip(whole["ratios"], _ratios64(kind, "fp32", 0.5)):
        assert float(((got.double() - ref) / ref).abs().max()) <= bound
    _check_bitwise_and_padding(kind, "fp32", 0.5, whole)


def _check_bitwise_and_padding(kind, gdt, grad_scale, whole):
    # per bucket == whole model, bit for bit; and run to run
    parts = _run(DEV, kind, gdt, grad_scale, per_bucket=True)
    again = _run(DEV, kind, gdt, grad_scale)
    for other in (parts, again):
        for k in whole:
            if k in ("ratios", "shadow"):
                continue
            assert _bits(whole[k], other[k]), k
        for a, b in zip(whole["ratios"], other["ratios"]):
            assert _bits(a, b)
    # the padding of the flat buffers stays exactly 0
    flat = make_flat(SHAPES6, bucket_bytes=BUCKET_BYTES)
    pad = torch.ones(flat.numel, dtype=torch.bool)
    for o, p in zip(flat.offsets, flat.params):
        pad[o:o + p.numel()] = False
    for k in ("p", "exp_avg", "exp_avg_sq", "mom"):
        if k in whole:
            assert bool((whole[k][pad] == 0).all()), k


@pytest.mark.parametrize("kind", ["lars", "lamb"])
def test_bf16_shadow_is_the_rounded_master(kind):
    ops.require()
    plain = _run(DEV, kind, "bf16", 0.5)
    sh = _run(DEV, kind, "bf16", 0.5, shadow=True)
    assert _bits(sh["p"], plain["p"])
    assert torch.equal(sh["shadow"].view(torch.int16), sh["p"].bfloat16().view(torch.int16))
    parts = _run(DEV, kind, "bf16", 0.5, per_bucket=True, shadow=True)
    assert torch.equal(parts["shadow"].view(torch.int16), sh["shadow"].view(torch.int16))


@pytest.mark.parametrize("kind", ["lars", "lamb"])
def test_two_launches_per_step_range(kind, monkeypatch):
    C = ops.require()
    flat = make_flat(SHAPES6, device=DEV, bucket_bytes=BUCKET_BYTES)
    opt = _opt(kind, flat)
    g = make_grad(flat, 0)
    calls = []
    for op, name in enumerate(("layerwise_stage", "layerwise_apply")):
        real = getattr(C, name)
        monkeypatch.setattr(ops._C, name,
                            lambda a, op=op, real=real: (calls.append(op), real(a))[1])
    opt.step(grad=g)  # the whole model: builds its plan
    assert calls == [0, 1]
    for b in flat.buckets:
        opt.step_range(b.start, b.length, g[b.start:b.start + b.length], 1.0)
    assert calls == [0, 1] * 3
    monkeypatch.undo()
    torch.cuda.synchronize()
    for start, length in [(0, flat.numel), (flat.buckets[1].start, flat.buckets[1].length)]:
        gr = torch.cuda.CUDAGraph(keep_graph=True)
        with torch.cuda.graph(gr, capture_error_mode="thread_local"):
            opt.step_range(start, length, g[start:start + length], 1.0)
        info = ops.graph_info(gr.raw_cuda_graph())
        assert info["linear"] and info["types"] == {"kernel": 2}, info


@pytest.mark.parametrize("kind", ["lars", "lamb"])
def test_graph_replays_follow_the_device_lr_and_step(kind):
    """Three replays of one captured step with an lr change between them are bitwise three eager
    steps: lr, t (LAMB's bias correction) and LARS's first-step flag are read on the device."""
    ops.require()
    lrs = [KW[kind]["lr"], KW[kind]["lr"] * 0.5, KW[kind]["lr"] * 0.125]
    eager_flat = make_flat(SHAPES6, device=DEV, bucket_bytes=BUCKET_BYTES)
    eager = _opt(kind, eager_flat)
    flat = make_flat(SHAPES6, device=DEV, bucket_bytes=BUCKET_BYTES)
    opt = _opt(kind, flat)
    p0 = flat.data.clone()
    sd0 = {k: (v.clone() if torch.is_tensor(v) else v) for k, v in opt.state_dict().items()}
    grads = [make_grad(flat, s) for s in range(3)]
    opt.step(grad=grads[0])  # an eager step builds the plan tables; then back to the start
    opt.load_state_dict(sd0)
    flat.data.copy_(p0)
    gbuf = torch.zeros_like(grads[0])
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, capture_error_mode="thread_local"):
        opt.step(grad=gbuf)
    opt.steps = 0  # the capture ran nothing
    for lr, gr in zip(lrs, grads):
        eager.lr = lr
        eager.step(grad=gr)
        opt.lr = lr
        gbuf.copy_(gr)
        g.replay()
        opt.steps += 1
    torch.cuda.synchronize()
    a, b = _state(eager_flat, eager), _state(flat, opt)
    for k in a:
        assert _bits(a[k], b[k]), k
    assert _bits(eager.ratio.cpu(), opt.ratio.cpu())
    assert int(opt.step_t) == 3


@pytest.mark.parametrize("kind", ["lars", "lamb"])
def test_host_step_count_equals_the_device_counter(kind):
    """``ops.layerwise_step`` without a device counter takes ``t`` / ``first`` from the host:
    LARS bitwise, LAMB to fp32 rounding of the bias corrections (python's and the device's pow)."""
    ops.require()
    fa = make_flat(SHAPES6, device=DEV, bucket_bytes=BUCKET_BYTES)
    fb = make_flat(SHAPES6, device=DEV, bucket_bytes=BUCKET_BYTES)
    a, b = _opt(kind, fa), _opt(kind, fb)
    lw = b._plan(0, fb.numel)
    kw = dict(KW[kind])
    for s in range(2):
        g = make_grad(fa, s)
        a.step(grad=g)
        if kind == "lars":
            ops.layerwise_step(lw, "lars", fb.data, g, b.mom, first=(s == 0), step=None, **kw)
        else:
            ops.layerwise_step(lw, "lamb", fb.data, g, b.exp_avg, b.exp_avg_sq, t=s + 1,
                               step=None, **kw)
    sa, sb = _state(fa, a), _state(fb, b)
    for k in sa:
        if kind == "lars":
            assert _bits(sa[k], sb[k]), k
        else:
            torch.testing.assert_close(sa[k], sb[k], rtol=1e-6, atol=1e-9, msg=k)
    assert not _bits(sa["p"], make_flat(SHAPES6, bucket_bytes=BUCKET_BYTES).data)


def test_wrapper_refusals_raise_before_any_launch():
    ops.require()
    flat = make_flat(SHAPES6, device=DEV, bucket_bytes=BUCKET_BYTES)
    opt = _opt("lamb", flat)
    lw = opt._plan(0, flat.numel)
    p, m, v = flat.data, opt.exp_avg, opt.exp_avg_sq
    g = make_grad(flat, 0)
    before = p.clone()
    with pytest.raises(ValueError, match="unknown layer-wise rule"):
        ops.layerwise_step(lw, "adam", p, g, m, v, lr=0.1)
    with pytest.raises(ValueError, match="needs exp_avg_sq"):
        ops.layerwise_step(lw, "lamb", p, g, m, None, lr=0.1)
    with pytest.raises(ValueError, match="the range needs"):
        ops.layerwise_step(lw, "lamb", p, g[:-64], m, v, lr=0.1)
    with pytest.raises(ValueError, match="aligned"):
        ops.layerwise_step(lw, "lamb", p, torch.zeros(flat.numel + 1, device=DEV)[1:], m, v, lr=0.1)
    with pytest.raises(TypeError):
        ops.layerwise_step(lw, "lamb", p, g.double(), m, v, lr=0.1)
    with pytest.raises(ValueError, match="must hold"):
        ops.LayerwisePlan(lw.plan, lw.adapt[:-1], lw.ratio, lw.partials)
    assert torch.equal(p, before)
