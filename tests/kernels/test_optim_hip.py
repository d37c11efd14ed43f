"""The flat optimizer, pack and cast kernels (``ops/csrc/optim.hip``: k_sgd_flat, k_adam_flat,
k_sgd_ptrs, k_pack_grads, k_cast_scale) on one MI355X against the independent fp32 / float64
reference of ``tests/optim_ref.py``.

Exactness contract.  SGD (flat and pointer table), the packed gradients, the casts, the bf16 shadow
and Adam with a host ``lr_step`` are bitwise ``ref32``: every product and sum is rounded on its
own on both sides (``-ffp-contract=off``) and the build's fp32 square root and divide are correctly
rounded.  Adam with the device step counter derives ``lr_step`` from ``pow`` in double, which is
not correctly rounded, so that path is held to ``ref64`` within ``optim_ref.limit``: four times
the CPU fp32 reference's own error, at least one ulp of the largest value.  Adam's parameters start
at ``|p0| ~ lr`` so that this bound resolves the update and not just the parameter: an off-by-one
step count moves ``lr_step`` by 25 % at t = 1 and double instead of fp32 betas by 6.7e-6, 26 times
the fp32 reference's error on these inputs.

Every buffer is a view ``LEAD + GUARD`` elements into a larger allocation (16 B aligned for fp32,
8 B for bf16 / fp16, and no better) between two runs of GUARD elements holding a fixed bit pattern,
which also fills the padding between the tensors of the pointer-table cases; all of it must be
bit-identical after the launches.

Sizes: 4, 1028 and 3076 elements, and 2 * 2,097,152 + 4 * 259 (the grid is capped at 2048 blocks
of 256 threads of 4 elements: every thread makes two trips of the stride loop, 259 a third)."""
import functools

import numpy as np
import pytest
import torch

from ewdml import ops
from ewdml.compress.plan import BucketPlan
from tests import optim_ref as R

pytestmark = pytest.mark.gpu

DEV = "cuda"
GUARD, LEAD = 64, 4
PAT32, PAT16 = 0x5A5A5A5A, 0x5A5A  # 1.5e16 as fp32 / bf16, 203.25 as fp16: non-zero, not NaN
SMALL = (4, 1028, 3076)
BIG = 2 * 2097152 + 4 * 259
DT = {"fp32": torch.float32, "bf16": torch.bfloat16, "fp16": torch.float16}
BF16 = torch.bfloat16


def _idt(dt):
    return torch.int32 if torch.empty((), dtype=dt).element_size() == 4 else torch.int16


def _bits(t):
    return t.contiguous().view(_idt(t.dtype))


def _same(a, b):
    return a.dtype == b.dtype and torch.equal(_bits(a.cpu()), _bits(b.cpu()))


def _ulps(a, b):
    """Largest distance in units of the last place (fp32 tensors of one sign pattern)."""
    return int((_bits(a.cpu()).long() - _bits(b.cpu()).long()).abs().max())


def _pattern(n, dt):
    """``n`` elements of the guard pattern on the CPU."""
    idt = _idt(dt)
    return torch.full((n,), PAT32 if idt == torch.int32 else PAT16, dtype=idt).view(dt)


class Buf:
    """Device copy of the 1-D CPU tensor ``values`` as the view ``v`` inside its guards."""

    def __init__(self, values):
        self.n, dt = values.numel(), values.dtype
        self.lo = LEAD + GUARD
        self.raw = _pattern(self.lo + self.n + GUARD, dt).to(DEV)
        self.v = self.raw[self.lo:self.lo + self.n]
        self.v.copy_(values)
        align = 16 if _idt(dt) == torch.int32 else 8
        assert self.v.data_ptr() % align == 0 and self.v.data_ptr() % (2 * align) != 0

    def cpu(self):
        return self.v.cpu()

    def guards_ok(self):
        r, pat = _bits(self.raw.cpu()), _bits(_pattern(1, self.raw.dtype))
        return bool((r[:self.lo] == pat).all()) and bool((r[self.lo + self.n:] == pat).all())


def _guards(**bufs):
    for name, b in bufs.items():
        for x in (b if isinstance(b, (list, tuple)) else [b]):
            assert x is None or x.guards_ok(), f"{name}: guard elements were written"


def _grads(gen, n, steps, gdt, damp_third=False):
    """Raw gradients with a per-step random scale, their values representable in ``gdt``; with
    ``damp_third`` the third is small, so that exp_avg_sq falls below its running maximum."""
    out = []
    for s in range(steps):
        scale = 0.1 + float(torch.rand(1, generator=gen))
        if damp_third and s == 2:
            scale *= 0.005
        out.append((torch.randn(n, generator=gen) * scale).to(DT[gdt]))
    return out


# ---- SGD over a flat range -----------------------------------------------------------------------
SGD_CASES = {
    "momentum0": dict(hp=dict(lr=0.1)),
    "first_wd": dict(hp=dict(lr=0.1, momentum=0.9, weight_decay=1e-3)),
    "dampening": dict(hp=dict(lr=0.1, momentum=0.9, dampening=0.1)),
    "nesterov_wd": dict(hp=dict(lr=0.05, momentum=0.9, weight_decay=1e-3, nesterov=True)),
    "scale_fp32": dict(hp=dict(lr=0.1, momentum=0.9, weight_decay=1e-3), grad_scale=1.0 / 3.0),
    "scale_bf16": dict(hp=dict(lr=0.1, momentum=0.9, weight_decay=1e-3), grad_scale=1.0 / 3.0,
                       gdt="bf16"),
    "scale_fp16": dict(hp=dict(lr=0.1, momentum=0.9, dampening=0.1), grad_scale=1.0 / 3.0,
                       gdt="fp16"),
    "lr_tensor": dict(hp=dict(lr=0.1, momentum=0.9, weight_decay=1e-3, nesterov=True),
                      lr_tensor=True),
}


@functools.lru_cache(maxsize=None)
def _sgd_ref(case, n, steps):
    """Inputs and the CPU references' final state (computed once per case)."""
    c = SGD_CASES[case]
    gen = torch.Generator().manual_seed(100 + n % 1000)
    p0, m0 = torch.randn(n, generator=gen), torch.randn(n, generator=gen)
    grads = _grads(gen, n, steps, c.get("gdt", "fp32"))
    p32, m32, p64, m64 = p0.clone(), m0.clone(), p0.double(), m0.double()
    for s, g in enumerate(grads):
        kw = dict(first=s == 0, grad_scale=c.get("grad_scale", 1.0), **c["hp"])
        R.sgd32(p32, m32, g, **kw)
        R.sgd64(p64, m64, g, **kw)
    return p0, m0, grads, (p32, m32), (p64, m64)


def _sgd_flat_case(case, n, steps):
    c = SGD_CASES[case]
    hp = dict(c["hp"])
    p0, m0, grads, (p32, m32), (p64, m64) = _sgd_ref(case, n, steps)
    p, m, sh = Buf(p0), Buf(m0), Buf(_pattern(n, BF16))
    lr_t = None
    if c.get("lr_tensor"):  # the device value is the rate; the host argument must be ignored
        lr_t = Buf(torch.tensor([hp["lr"]], dtype=torch.float32))
        hp["lr"] = 77.0
    gb = [Buf(g) for g in grads]
    for s, g in enumerate(gb):
        ops.sgd_flat(p.v, m.v, g.v, grad_scale=c.get("grad_scale", 1.0), first=s == 0,
                     shadow=sh.v, lr_tensor=None if lr_t is None else lr_t.v, **hp)
    torch.cuda.synchronize()
    tag = f"sgd {case} n={n} "
    print(f"{tag}p {_ulps(p.cpu(), p32)} ulp, mom {_ulps(m.cpu(), m32)} ulp from ref32")
    assert _same(p.cpu(), p32), tag + "p"
    assert _same(m.cpu(), m32), tag + "mom"
    assert _same(sh.cpu(), p32.to(BF16)), tag + "shadow"
    assert not _same(p.cpu(), p0)
    if hp.get("momentum", 0.0) == 0.0:
        assert _same(m.cpu(), m0)  # never touched
    R.check("p", p.cpu(), p32, p64, tag)
    R.check("mom", m.cpu(), m32, m64, tag)
    _guards(p=p, m=m, sh=sh, g=gb, lr_t=lr_t)
    assert all(_same(g.cpu(), g0) for g, g0 in zip(gb, grads))  # only read


@pytest.mark.parametrize("case", list(SGD_CASES))
def test_sgd_flat_is_ref32_bitwise(case):
    """Three steps, ``first`` on the first only, at every small size."""
    ops.require()
    for n in SMALL:
        _sgd_flat_case(case, n, 3)


def test_sgd_flat_stride_loop():
    ops.require()
    _sgd_flat_case("scale_fp32", BIG, 2)
    _sgd_ref.cache_clear()  # the large reference is of no use to another test


# ---- Adam / AMSGrad over a flat range ------------------------------------------------------------
ADAM = dict(lr=1e-3, beta1=0.9, beta2=0.999, eps=1e-8, weight_decay=1e-2)
ADAM_KERNEL = {k: v for k, v in ADAM.items() if k != "lr"}
NAMES = ("p", "exp_avg", "exp_avg_sq", "max_exp_avg_sq")


@functools.lru_cache(maxsize=None)
def _adam_ref(n, amsgrad, gdt, grad_scale, lrs):
    """Inputs and both CPU references after ``len(lrs)`` steps at those base rates; ``ref32``
    takes each step's ``lr_step`` from the fp32-rounded betas, as a correct kernel does."""
    gen = torch.Generator().manual_seed(200 + n % 1000)
    p0 = torch.randn(n, generator=gen) * ADAM["lr"]  # |p0| ~ lr
    grads = _grads(gen, n, len(lrs), gdt, damp_third=True)
    s32 = [p0.clone()] + [torch.zeros(n) for _ in range(3)]
    s64 = [p0.double()] + [torch.zeros(n, dtype=torch.float64) for _ in range(3)]
    for t, (g, lr) in enumerate(zip(grads, lrs), start=1):
        step = R.lr_step64(lr, ADAM["beta1"], ADAM["beta2"], t)
        R.adam32(*s32, g, step, amsgrad=amsgrad, grad_scale=grad_scale, **ADAM_KERNEL)
        R.adam64(*s64, g, t, amsgrad=amsgrad, grad_scale=grad_scale, **dict(ADAM, lr=lr))
    return p0, grads, s32, s64


def _adam_state(p0, vmax=True):
    n = p0.numel()
    z = torch.zeros(n)
    return [Buf(p0), Buf(z), Buf(z), Buf(z) if vmax else None]


def _adam_compare(tag, state, s32, s64, amsgrad, bitwise):
    got = [b.cpu() for b in state[:4 if amsgrad else 3]]
    for name, x, x32 in zip(NAMES, got, s32):
        print(f"{tag}{name}: {_ulps(x, x32)} ulp from ref32")
    for name, x, x32, x64 in zip(NAMES, got, s32, s64):
        R.check(name, x, x32, x64, tag)
    if bitwise:
        for name, x, x32 in zip(NAMES, got, s32):
            assert _same(x, x32), tag + name
    return got


HOST_CASES = {  # amsgrad, gradient dtype, grad_scale, max_exp_avg_sq supplied
    "adam": (False, "fp32", 1.0, False),
    "adam_spare_max": (False, "fp32", 1.0 / 3.0, True),
    "amsgrad": (True, "fp32", 1.0, True),
    "adam_bf16": (False, "bf16", 1.0 / 3.0, False),
    "amsgrad_fp16": (True, "fp16", 1.0 / 3.0, True),
}


@pytest.mark.parametrize("case", list(HOST_CASES))
def test_adam_flat_host_step_is_ref32_bitwise(case):
    """``step=None``: the kernel takes ``lr_step`` as given (here from the fp32-rounded betas)."""
    ops.require()
    amsgrad, gdt, grad_scale, with_max = HOST_CASES[case]
    for n in SMALL:
        p0, grads, s32, s64 = _adam_ref(n, amsgrad, gdt, grad_scale, (ADAM["lr"],) * 3)
        state = _adam_state(p0, with_max)
        spare = torch.randn(n)
        if with_max and not amsgrad:
            state[3] = Buf(spare)  # a supplied buffer that the plain rule must not touch
        sh = Buf(_pattern(n, BF16))
        gb = [Buf(g) for g in grads]
        for t, g in enumerate(gb, start=1):
            step = R.lr_step64(ADAM["lr"], ADAM["beta1"], ADAM["beta2"], t)
            ops.adam_flat(state[0].v, state[1].v, state[2].v,
                          None if state[3] is None else state[3].v, g.v, step,
                          grad_scale=grad_scale, amsgrad=amsgrad, shadow=sh.v, **ADAM_KERNEL)
        torch.cuda.synchronize()
        got = _adam_compare(f"adam host {case} n={n} ", state, s32, s64, amsgrad, bitwise=True)
        assert _same(sh.cpu(), got[0].to(BF16)) and not _same(got[0], p0)
        if amsgrad:
            assert n == 4 or float((got[3] > got[2]).float().mean()) > 0.5  # the maximum is used
        elif with_max:
            assert _same(state[3].cpu(), spare)
        _guards(state=state, sh=sh, g=gb)


def _device_steps(n, amsgrad, gdt, grad_scale, use_lr_tensor, steps=3):
    p0, grads, s32, s64 = _adam_ref(n, amsgrad, gdt, grad_scale, (ADAM["lr"],) * steps)
    state = _adam_state(p0, amsgrad)
    sh = Buf(_pattern(n, BF16))
    step_t = Buf(torch.zeros(1, dtype=torch.int32))
    lr_t = Buf(torch.tensor([ADAM["lr"]], dtype=torch.float32)) if use_lr_tensor else None
    gb = [Buf(g) for g in grads]
    for g in gb:
        ops.adam_flat(state[0].v, state[1].v, state[2].v,
                      None if state[3] is None else state[3].v, g.v, 77.0,
                      grad_scale=grad_scale, amsgrad=amsgrad, shadow=sh.v, step=step_t.v,
                      lr=77.0 if use_lr_tensor else ADAM["lr"],
                      lr_tensor=None if lr_t is None else lr_t.v, **ADAM_KERNEL)
        step_t.v.add_(1)
    torch.cuda.synchronize()
    assert int(step_t.cpu()) == steps
    tag = f"adam device {'lr_tensor' if use_lr_tensor else 'host lr'} amsgrad={amsgrad} n={n} "
    got = _adam_compare(tag, state, s32, s64, amsgrad, bitwise=False)
    assert _same(sh.cpu(), got[0].to(BF16))
    _guards(state=state, sh=sh, g=gb, step_t=step_t, lr_t=lr_t)


@pytest.mark.parametrize("use_lr_tensor", [False, True])
def test_adam_flat_device_step_follows_ref64(use_lr_tensor):
    """The path the trainer runs: t = counter + 1 and the base rate are read on the device, the
    ``lr_step`` argument (and with ``lr_tensor`` the host ``lr``) is a wrong value on purpose."""
    ops.require()
    amsgrad = use_lr_tensor  # Adam with the host rate, AMSGrad with the device rate
    for n in SMALL:
        _device_steps(n, amsgrad, "fp32", 1.0, use_lr_tensor)


def test_adam_flat_stride_loop():
    ops.require()
    _device_steps(BIG, True, "fp32", 1.0, True, steps=2)
    _adam_ref.cache_clear()


def test_adam_flat_graph_replays_follow_the_device_step_and_lr():
    """One captured launch plus the counter's increment, replayed four times with the device
    rate changed before the third, is four float64 steps at those rates."""
    ops.require()
    n, lr2 = 3076, 2.5e-4
    lrs = (ADAM["lr"], ADAM["lr"], lr2, lr2)
    p0, grads, s32, s64 = _adam_ref(n, True, "fp32", 1.0, lrs)
    state = _adam_state(p0)
    sh = Buf(_pattern(n, BF16))
    step_t = Buf(torch.zeros(1, dtype=torch.int32))
    lr_t = Buf(torch.tensor([lrs[0]], dtype=torch.float32))
    g = Buf(grads[0])

    def launch():
        ops.adam_flat(state[0].v, state[1].v, state[2].v, state[3].v, g.v, 77.0, amsgrad=True,
                      shadow=sh.v, step=step_t.v, lr=77.0, lr_tensor=lr_t.v, **ADAM_KERNEL)
        step_t.v.add_(1)

    launch()  # warm-up, then back to the start
    state[0].v.copy_(p0)
    for b in state[1:]:
        b.v.zero_()
    step_t.v.zero_()
    torch.cuda.synchronize()
    gr = torch.cuda.CUDAGraph(keep_graph=True)
    with torch.cuda.graph(gr, capture_error_mode="thread_local"):
        launch()
    info = ops.graph_info(gr.raw_cuda_graph())
    assert info["linear"] and info["types"] == {"kernel": 2}, info
    gr.instantiate()
    for s, (gs, lr) in enumerate(zip(grads, lrs)):
        g.v.copy_(gs)
        if s == 2:
            lr_t.v.fill_(lr)
        gr.replay()
    torch.cuda.synchronize()
    assert int(step_t.cpu()) == 4
    got = _adam_compare("adam graph ", state, s32, s64, True, bitwise=False)
    assert _same(sh.cpu(), got[0].to(BF16))
    _guards(state=state, sh=sh, g=g, step_t=step_t, lr_t=lr_t)


# ---- pointer-table kernels -----------------------------------------------------------------------
# tails of 1, 2 and 3 elements in both gradient dtypes, exactly one chunk, a chunk plus one
NUMELS = [1, 3, 5, 8191, 8192, 8193, 32770, 8199, 2]
GRAD_DT = [torch.float32] * 7 + [BF16] * 2


def _plan():
    offs, o = [], 0
    for n in NUMELS:
        offs.append(o)
        o += (n + 63) // 64 * 64
    return BucketPlan(NUMELS, offs, 1.0, 0, o)


PLAN = _plan()
INSIDE = torch.zeros(PLAN.length, dtype=torch.bool)
for _o, _n in zip(PLAN.offsets, PLAN.numels):
    INSIDE[_o:_o + _n] = True
TENSORS = list(zip(PLAN.offsets, PLAN.numels))


def _bucket(values, dt=torch.float32):
    """A bucket-long CPU tensor: ``values`` (one per tensor) at the plan's offsets, the guard
    pattern between them."""
    out = _pattern(PLAN.length, dt)
    for (o, n), x in zip(TENSORS, values):
        out[o:o + n] = x.to(dt)
    return out


def _padding_ok(t):
    return bool((_bits(t)[~INSIDE] == _bits(_pattern(1, t.dtype))).all())


@functools.lru_cache(maxsize=None)
def _bucket_inputs():
    gen = torch.Generator().manual_seed(300)
    grads = [(torch.randn(n, generator=gen) * (0.1 + float(torch.rand(1, generator=gen)))).to(dt)
             for n, dt in zip(NUMELS, GRAD_DT)]
    p0 = [torch.randn(n, generator=gen) for n in NUMELS]
    m0 = [torch.randn(n, generator=gen) for n in NUMELS]
    return grads, p0, m0


PTR_CASES = {
    "first": dict(hp=dict(lr=0.1, momentum=0.9, weight_decay=1e-3), first=True),
    "nesterov_wd_scale": dict(hp=dict(lr=0.05, momentum=0.9, weight_decay=1e-3, nesterov=True),
                              first=False, grad_scale=1.0 / 3.0),
    "lr_tensor": dict(hp=dict(lr=0.05, momentum=0.9, dampening=0.1), first=False, lr_tensor=True),
}


@pytest.mark.parametrize("case", list(PTR_CASES))
def test_sgd_ptrs_is_ref32_bitwise_per_tensor(case):
    ops.require()
    c = PTR_CASES[case]
    hp, scale = dict(c["hp"]), c.get("grad_scale", 1.0)
    grads, p0, m0 = _bucket_inputs()
    p32, m32 = [x.clone() for x in p0], [x.clone() for x in m0]
    for p, m, g in zip(p32, m32, grads):
        R.sgd32(p, m, g, first=c["first"], grad_scale=scale, **hp)
    dp = ops.DevicePlan(PLAN, DEV)
    p, m, sh = Buf(_bucket(p0)), Buf(_bucket(m0)), Buf(_pattern(PLAN.length, BF16))
    gb = [Buf(g) for g in grads]
    lr_t = None
    if c.get("lr_tensor"):
        lr_t = Buf(torch.tensor([hp["lr"]], dtype=torch.float32))
        hp["lr"] = 77.0
    ops.sgd_ptrs(dp, [g.v for g in gb], p.v, m.v, grad_scale=scale, first=c["first"],
                 shadow=sh.v, lr_tensor=None if lr_t is None else lr_t.v, **hp)
    torch.cuda.synchronize()
    pc, mc, sc = p.cpu(), m.cpu(), sh.cpu()
    for i, (o, n) in enumerate(TENSORS):
        assert _same(pc[o:o + n], p32[i]), f"p of tensor {i} ({n})"
        assert _same(mc[o:o + n], m32[i]), f"mom of tensor {i} ({n})"
        assert _same(sc[o:o + n], p32[i].to(BF16)), f"shadow of tensor {i} ({n})"
        assert not _same(pc[o:o + n], p0[i])
    assert _padding_ok(pc) and _padding_ok(mc) and _padding_ok(sc)
    _guards(p=p, m=m, sh=sh, g=gb, lr_t=lr_t)
    assert all(_same(g.cpu(), g0) for g, g0 in zip(gb, grads))


@pytest.mark.parametrize("source", ["list", "flat"])
@pytest.mark.parametrize("dst", ["fp32", "bf16", "fp16"])
def test_pack_grads_is_the_scaled_cast_bitwise(dst, source):
    """Per-tensor gradients (fp32 and bf16) or the bucket's flat fp32 view into every wire dtype."""
    ops.require()
    grads = _bucket_inputs()[0]
    dp = ops.DevicePlan(PLAN, DEV)
    third = torch.tensor(1.0 / 3.0, dtype=torch.float32)
    out = Buf(_pattern(PLAN.length, DT[dst]))
    if source == "list":
        gb = [Buf(g) for g in grads]
        ops.pack_grads(dp, [g.v for g in gb], out.v, 1.0 / 3.0)
    else:
        gb = [Buf(_bucket(grads))]
        ops.pack_grads(dp, gb[0].v, out.v, 1.0 / 3.0)
    torch.cuda.synchronize()
    oc = out.cpu()
    for i, ((o, n), g) in enumerate(zip(TENSORS, grads)):
        assert _same(oc[o:o + n], (g.float() * third).to(DT[dst])), f"tensor {i} ({n})"
    assert _padding_ok(oc)
    _guards(out=out, g=gb)


# ---- the wire cast -------------------------------------------------------------------------------
# every upper half (all exponents, both signs, subnormals, inf, NaNs) with lower halves on both
# sides of the bf16 tie (0x8000) and of the fp16 tie (13 dropped bits: 0x1000 under an even kept
# bit, 0x3000 under an odd one; further down in fp16's subnormal range)
LOWER = (0x0000, 0x0fff, 0x1000, 0x1001, 0x3000, 0x7fff, 0x8000, 0x8001, 0xffff)


def _cast_case(x, scale, dst):
    want = (x * torch.tensor(scale, dtype=torch.float32)).to(DT[dst])
    src, out = Buf(x), Buf(_pattern(x.numel(), DT[dst]))
    ops.cast_scale(src.v, out.v, scale)
    torch.cuda.synchronize()
    got = out.cpu()
    nan = torch.isnan(want)
    bad = (_bits(got) != _bits(want)) & ~nan
    assert not bool(bad.any()), \
        f"{dst} * {scale}: {int(bad.sum())} differ, first inputs " \
        f"{[hex(int(v) & 0xffffffff) for v in _bits(x)[bad][:8]]}"
    assert bool(torch.isnan(got[nan]).all())  # the kernel keeps a NaN's sign and payload
    _guards(src=src, out=out)
    assert _same(src.cpu(), x)
    return want, nan


@pytest.mark.parametrize("scale", [1.0, 0.25])
@pytest.mark.parametrize("dst", ["bf16", "fp16"])
def test_cast_scale_every_exponent_and_tie(dst, scale):
    ops.require()
    hi = np.arange(65536, dtype=np.uint32)[:, None] << 16
    x = torch.from_numpy((hi | np.array(LOWER, dtype=np.uint32)[None, :]).reshape(-1)
                         .view(np.int32).copy()).view(torch.float32)
    want, nan = _cast_case(x, scale, dst)
    assert int(nan.sum()) >= 2 * 127 * len(LOWER) - 2 and bool(torch.isinf(want).any())
    assert bool(((want != 0) & (want.float().abs() < (2.0 ** -126 if dst == "bf16"
                                                      else 2.0 ** -14))).any())  # subnormals


@pytest.mark.parametrize("dst", ["bf16", "fp16"])
def test_cast_scale_stride_loop(dst):
    ops.require()
    x = torch.randn(BIG, generator=torch.Generator().manual_seed(400)) * 100
    _cast_case(x, 0.25, dst)


# ---- operand checks ------------------------------------------------------------------------------
def test_bad_operands_rejected():
    """Dtype and size are checked on the host, before any launch."""
    ops.require()
    n = 8
    p, m, v, vm, g = (torch.zeros(n, device=DEV) for _ in range(5))
    g.fill_(1.0)
    out = torch.zeros(n, dtype=BF16, device=DEV)
    hp = dict(beta1=0.9, beta2=0.999, eps=1e-8)
    with pytest.raises(TypeError):  # a gradient dtype the kernels do not read
        ops.adam_flat(p, m, v, None, g.double(), 1e-3, **hp)
    with pytest.raises(TypeError):
        ops.sgd_flat(p, m, g.double(), 0.1)
    with pytest.raises(ValueError):  # AMSGrad writes n floats through max_exp_avg_sq
        ops.adam_flat(p, m, v, None, g, 1e-3, amsgrad=True, **hp)
    with pytest.raises(ValueError):
        ops.adam_flat(p, m, v, vm[:4], g, 1e-3, amsgrad=True, **hp)
    with pytest.raises(ValueError):
        ops.adam_flat(p, m, v, torch.zeros(n + 4, device=DEV), g, 1e-3, amsgrad=True, **hp)
    with pytest.raises(ValueError):  # 16-byte accesses: n % 4 == 0
        ops.sgd_flat(p[:6], m[:6], g[:6], 0.1)
    with pytest.raises(ValueError):
        ops.adam_flat(p[:6], m[:6], v[:6], None, g[:6], 1e-3, **hp)
    with pytest.raises(ValueError):
        ops.cast_scale(g[:6], out[:6], 1.0)
    torch.cuda.synchronize()
    for t in (p, m, v, vm, out):
        assert not t.any()  # nothing ran
