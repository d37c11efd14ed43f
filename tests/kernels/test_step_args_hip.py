"""The receive-side step shared by every fused decode (ops._step -> the extension's StepArgs), on
one MI355X: each codec's ``*_decode_apply`` wrapper driven through the step's three shapes on one
small bucket, bitwise against ``oracle.decode_sum`` + ``oracle.sgd_apply``.

Every call rejected here is rejected by the Python wrapper, before anything is launched; the
extension's own check (``ew_step_check``) is exercised on the CPU by tests/unit/test_step_check.py."""
import pytest
import torch

from ewdml import ops
from ewdml.compress import oracle
from ewdml.compress.plan import BucketPlan, Layout
from ewdml.compress.rng import stream_key

pytestmark = pytest.mark.gpu

DEV = "cuda"
# a full chunk, a tail chunk that is no multiple of 4, and a tensor smaller than a chunk
NUMELS = (8192 + 5, 37)
N = 2
LEVELS = 127
ROT_KEY = oracle.hsign_rot_key(3, 1)
SEED, STEP, RANK = 5, 41, 3
# lr = 2^-4 and dampening = 0: lr * d and (1 - dampening) * d are exact, so the reference does not
# depend on whether torch's CPU ``add_(x, alpha=)`` contracts its multiply-add (the kernels never
# do); every other step of oracle.sgd_apply is a separately rounded operation
HP = dict(lr=0.0625, momentum=0.9, dampening=0.0, weight_decay=5e-4, nesterov=False)
HP_PLAIN = dict(lr=0.0625, momentum=0.0, dampening=0.0, weight_decay=0.0, nesterov=False)

# name: (layout kind, bits, encode(dp, grad, payload, layout, rank), decode wrapper and its
# codec-specific arguments, rot_key of oracle.decode_sum, the kernel needs the momentum buffer)
CODECS = {
    "topk_qsgd8": ("topk_qsgd", 8,
                   lambda dp, g, pay, lay, r: ops.topk_encode(dp, g, pay, lay, LEVELS, "max",
                                                              stream_key(SEED, STEP, r)),
                   ops.topk_decode_apply, (LEVELS,), {}, None, False),
    "qsgd8": ("qsgd", 8,
              lambda dp, g, pay, lay, r: ops.qsgd_encode(dp, g, pay, lay, LEVELS, "max",
                                                         stream_key(SEED, STEP, r)),
              ops.qsgd_decode_apply, (LEVELS,), {}, None, True),
    "sign": ("sign", 8, lambda dp, g, pay, lay, r: ops.sign_encode(dp, g, pay, lay),
             ops.sign_decode_apply, (), {}, None, False),
    "sign_rot": ("sign", 8,
                 lambda dp, g, pay, lay, r: ops.sign_encode(dp, g, pay, lay, rot_key=ROT_KEY),
                 ops.sign_decode_apply, (), dict(rot_key=ROT_KEY), ROT_KEY, False),
    "mxfp8": ("mx", 8, lambda dp, g, pay, lay, r: ops.mx_encode(dp, g, pay, lay),
              ops.mx_decode_apply, (), {}, None, False),
    "tern": ("tern", 8,
             lambda dp, g, pay, lay, r: ops.tern_encode(dp, g, pay, lay, 2.5,
                                                        stream_key(SEED, STEP, r)),
             ops.tern_decode_apply, (), {}, None, False),
}


def _bits(t):
    return t.contiguous().view(torch.int32)


_CASES = {}


def _case(name):
    """(plan, layout, device plan, received rows on the device, their decoded mean, p0, m0),
    computed once per codec and only read."""
    if name not in _CASES:
        kind, bits, encode = CODECS[name][:3]
        offs, o = [], 0
        for n in NUMELS:
            offs.append(o)
            o += (n + 63) // 64 * 64
        plan = BucketPlan(list(NUMELS), offs, 0.05, 4096, o)
        lay = Layout.build(kind, plan, bits)
        dp = ops.DevicePlan(plan, DEV)
        gen = torch.Generator().manual_seed(17)
        recv = torch.zeros(N, lay.nbytes, dtype=torch.uint8, device=DEV)
        for r in range(N):  # the ranks' gradients differ in magnitude: the sum's order matters
            g = torch.zeros(plan.length)
            for off, n in zip(plan.offsets, plan.numels):
                g[off:off + n] = torch.randn(n, generator=gen) * (0.1 * 3.0 ** r)
            encode(dp, g.to(DEV), recv[r], lay, r)
        mean = oracle.decode_sum(recv.cpu(), plan, lay, LEVELS, 1.0 / N, CODECS[name][6])
        p0 = torch.randn(plan.length, generator=gen)
        m0 = torch.randn(plan.length, generator=gen)
        _CASES[name] = (plan, lay, dp, recv, mean, p0, m0)
    return _CASES[name]


def _decode(name, **kw):
    _, lay, dp, recv = _case(name)[:4]
    fn, args, extra = CODECS[name][3:6]
    fn(dp, recv, lay, *args, grad_scale=1.0 / N, **extra, **kw)


def _stepped(plan, mean, p0, m0, hp, first):
    p, m = p0.clone(), None if m0 is None else m0.clone()
    for off, n in zip(plan.offsets, plan.numels):
        oracle.sgd_apply(p[off:off + n], None if m is None else m[off:off + n],
                         mean[off:off + n], first=first, **hp)
    return p, m


@pytest.mark.parametrize("name", list(CODECS))
def test_grad_out_only(name):
    ops.require()
    plan, _, _, _, mean, _, _ = _case(name)
    go = torch.full((plan.length,), float("nan"), device=DEV)
    _decode(name, grad_out=go)
    got = go.cpu()
    assert mean.abs().max() > 0
    for off, n in zip(plan.offsets, plan.numels):
        assert torch.equal(_bits(got[off:off + n]), _bits(mean[off:off + n]))


@pytest.mark.parametrize("first", [True, False], ids=["first", "later"])
@pytest.mark.parametrize("name", list(CODECS))
def test_apply_with_momentum_shadow_device_lr_and_key(name, first):
    ops.require()
    plan, _, _, _, mean, p0, m0 = _case(name)
    p, m = _stepped(plan, mean, p0, m0, HP, first)
    pd, md = p0.to(DEV), m0.to(DEV)
    sh = torch.zeros(plan.length, dtype=torch.bfloat16, device=DEV)
    ks = torch.tensor([STEP, 0], dtype=torch.int32, device=DEV)
    lr_t = torch.tensor([HP["lr"]], device=DEV)  # the device scalar wins over the host value
    _decode(name, param=pd, mom=md, first=first, shadow=sh, key_state=ks, key_seed=SEED,
            key_rank=RANK, lr_tensor=lr_t, **dict(HP, lr=999.0))
    assert torch.equal(_bits(pd.cpu()), _bits(p))  # the positions between tensors included
    assert torch.equal(_bits(md.cpu()), _bits(m))
    for off, n in zip(plan.offsets, plan.numels):
        assert torch.equal(sh[off:off + n].cpu(), p[off:off + n].to(torch.bfloat16))
    assert [int(v) & 0xFFFFFFFF for v in ks.cpu()] == [STEP + 1,
                                                       stream_key(SEED, STEP + 1, RANK)]


def _assert_rejected(name, bufs, **kw):
    """The wrapper raises ValueError naming the momentum buffer, and nothing ran."""
    before = [t.clone() for t in bufs]
    with pytest.raises(ValueError, match="momentum buffer"):
        _decode(name, **kw)
    torch.cuda.synchronize()
    for t, b in zip(bufs, before):
        assert torch.equal(t, b)


@pytest.mark.parametrize("name", list(CODECS))
def test_apply_without_momentum_buffer(name):
    ops.require()
    plan, _, _, _, mean, p0, m0 = _case(name)
    pd, md = p0.to(DEV), m0.to(DEV)  # md is never passed: it must stay as it is
    go = torch.full((plan.length,), 7.0, device=DEV)
    sh = p0.to(torch.bfloat16).to(DEV)  # the sparse top-k step rewrites the sent positions only
    bufs = (pd, md, go, sh)
    # a momentum step without its buffer: every wrapper refuses
    _assert_rejected(name, bufs, param=pd, mom=None, grad_out=go, shadow=sh, **HP)
    _assert_rejected(name, bufs, param=pd, mom=None, grad_out=go, shadow=sh,
                     **dict(HP_PLAIN, nesterov=True))
    if CODECS[name][7]:  # the kernel reads the buffer whatever the momentum is
        _assert_rejected(name, bufs, param=pd, mom=None, grad_out=go, shadow=sh, **HP_PLAIN)
        return
    p, _ = _stepped(plan, mean, p0, None, HP_PLAIN, False)
    _decode(name, param=pd, mom=None, shadow=sh, **HP_PLAIN)
    assert torch.equal(_bits(pd.cpu()), _bits(p))
    assert torch.equal(md.cpu(), m0) and bool((go == 7.0).all())
    for off, n in zip(plan.offsets, plan.numels):
        assert torch.equal(sh[off:off + n].cpu(), p[off:off + n].to(torch.bfloat16))
