"""1-bit Adam's HIP kernels (ops/csrc/sign_codec.hip: the momentum mode of k_sign_encode and
k_sign_decode_onebit) vs the torch oracle, on one MI355X.

Exactness contract: payload bytes, residuals, the averaged momentum and -- with a host lr_step --
the parameters are bitwise the oracle's (``oracle.encode_sign_momentum`` /
``oracle.onebit_adam_apply``): every operation is rounded separately on both sides, sqrtf and the
divide are IEEE, and the file set is built with -ffp-contract=off.
"""
import pytest
import torch

from ewdml import ops
from ewdml.compress import oracle
from ewdml.compress.plan import BucketPlan, Layout
from ewdml.compress.rng import stream_key

pytestmark = pytest.mark.gpu

DEV = "cuda"

# one-element tensor and a tail shorter than a word | tails of 1..5 | a 5-element tail after full
# chunks, multi-chunk tensors
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


def _bits_equal(a, b):
    return torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def _split(plan, g, dtype=torch.float32):
    return [g[o:o + n].clone().to(dtype).to(DEV) for o, n in zip(plan.offsets, plan.numels)]


@pytest.mark.parametrize("wd", [0.0, 5e-4])
@pytest.mark.parametrize("beta1", [0.0, 0.9])
@pytest.mark.parametrize("numels", SHAPES)
def test_momentum_encode_matches_oracle(numels, beta1, wd):
    ops.require()
    plan = _plan(numels)
    lay = Layout.build("sign", plan)
    dp = ops.DevicePlan(plan, DEV)
    pay = torch.full((lay.nbytes,), 0xFF, dtype=torch.uint8, device=DEV)  # padding is rewritten
    m, p = _grad(plan, seed=70) * 2.0, _grad(plan, seed=71) * 30.0
    m_dev, p_dev = m.to(DEV), p.to(DEV)
    r_ref = _grad(plan, seed=50) * 0.3
    r_dev = r_ref.to(DEV)
    for it in range(2):
        g = _grad(plan, seed=len(numels) + it)
        g_dev = g.to(DEV)
        ref = oracle.encode_sign_momentum(g.clone(), plan, lay, r_ref, m, beta1, wd, p)
        ops.sign_encode_momentum(dp, g_dev, pay, lay, r_dev, m_dev, beta1, wd, p_dev)
        got = pay.cpu()
        assert torch.equal(got, ref), \
            f"encode {it}: payload differs at {(got != ref).nonzero()[:10].flatten()}"
        assert _bits_equal(r_dev.cpu(), r_ref), f"encode {it}: residual"
        assert _bits_equal(g_dev.cpu(), g) and _bits_equal(m_dev.cpu(), m)
        assert _bits_equal(p_dev.cpu(), p)
    if beta1 == 0.0 and wd == 0.0:  # the plain sign encode of the same g and residual
        r2 = _grad(plan, seed=50) * 0.3
        for it in range(2):
            ref = oracle.encode_sign(_grad(plan, seed=len(numels) + it), plan, lay, r2)
        assert torch.equal(pay.cpu(), ref) and _bits_equal(r_dev.cpu(), r2)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_momentum_encode_from_per_tensor_pointers(dtype):
    ops.require()
    plan = _plan([8192 + 7, 64, 30000, 5], bucket_offset=256)
    lay = Layout.build("sign", plan)
    g = _grad(plan, seed=3)
    for o, n in zip(plan.offsets, plan.numels):  # the flat reference holds the same values
        g[o:o + n] = g[o:o + n].to(dtype).float()
    dp = ops.DevicePlan(plan, DEV)
    pay = torch.zeros(lay.nbytes, dtype=torch.uint8, device=DEV)
    grads = _split(plan, g, dtype)
    before = [t.clone() for t in grads]
    m, p = _grad(plan, seed=9), _grad(plan, seed=10)
    m_dev, p_dev = m.to(DEV), p.to(DEV)
    r_ref = _grad(plan, seed=8) * 0.05
    r_dev = r_ref.to(DEV)
    for wd in (0.0, 5e-4):
        ref = oracle.encode_sign_momentum(g.clone(), plan, lay, r_ref, m, 0.9, wd, p)
        ops.sign_encode_momentum(dp, grads, pay, lay, r_dev, m_dev, 0.9, wd, p_dev)
        assert torch.equal(pay.cpu(), ref)
        assert _bits_equal(r_dev.cpu(), r_ref)
    for a, b in zip(grads, before):
        assert torch.equal(a, b)
    assert _bits_equal(m_dev.cpu(), m)


def _payloads(plan, lay, N, seed=100):
    # very different magnitudes per rank: the rank order of the fp32 sum matters
    return torch.stack([oracle.encode_sign(_grad(plan, seed=seed + r) * (3.0 ** r), plan, lay)
                        for r in range(N)])


def _apply_case(N):
    plan = _plan([20 * 25, 20, 8192 * 2 + 3, 1, 70001], bucket_offset=128)
    lay = Layout.build("sign", plan)
    recv = _payloads(plan, lay, N)
    gen = torch.Generator().manual_seed(11)
    p0 = torch.randn(plan.length, generator=gen)
    v0 = torch.rand(plan.length, generator=gen) * 1e-3
    v0[::5] = 0.0  # coordinates that never saw a gradient
    v0[3::7] = 1e-42  # denormal variances take the step
    m0 = torch.full((plan.length,), float("nan"))
    return plan, lay, recv, p0, m0, v0


@pytest.mark.parametrize("N", [1, 2, 4, 11])
def test_decode_apply_matches_oracle(N):
    ops.require()
    plan, lay, recv, p0, m0, v0 = _apply_case(N)
    lr_step, eps = 1e-3 * 0.7071 / 0.19, 1e-8
    p, m, v = p0.clone(), m0.clone(), v0.clone()
    oracle.onebit_adam_apply(recv, plan, lay, p, m, v, 1.0 / N, lr_step, eps)
    dp = ops.DevicePlan(plan, DEV)
    pd, md, vd = p0.to(DEV), m0.to(DEV), v0.to(DEV)
    sh = torch.zeros(plan.length, dtype=torch.bfloat16, device=DEV)
    seed, step, rank = 5, 41, 3
    ks = torch.tensor([step, 0], dtype=torch.int32, device=DEV)
    ops.sign_decode_onebit(dp, recv.to(DEV), lay, pd, md, vd, 1.0 / N, lr_step, eps,
                           freeze_step=4, shadow=sh, key_state=ks, key_seed=seed, key_rank=rank)
    inside = torch.zeros(plan.length, dtype=torch.bool)
    for off, n in zip(plan.offsets, plan.numels):
        inside[off:off + n] = True
    got_p, got_m = pd.cpu(), md.cpu()
    assert _bits_equal(got_m[inside], m[inside])
    assert _bits_equal(got_m[inside], oracle.decode_sum(recv, plan, lay, 0, 1.0 / N)[inside])
    ulp = (got_p.view(torch.int32) - p.view(torch.int32)).abs().max()
    print(f"max param difference: {int(ulp)} ulp")
    assert _bits_equal(got_p, p)
    assert _bits_equal(vd.cpu(), v0)  # the frozen variance is only read
    assert torch.isnan(got_m[~inside]).all() and _bits_equal(got_p[~inside], p0[~inside])
    still = inside & (v0 == 0)
    moved = inside & (v0 > 0)
    assert _bits_equal(got_p[still], p0[still]) and bool((got_p[moved] != p0[moved]).any())
    assert torch.isfinite(got_m[still]).all() and bool((got_m[still] != 0).all())
    for o, n in zip(plan.offsets, plan.numels):
        assert torch.equal(sh[o:o + n], pd[o:o + n].to(torch.bfloat16))
    got = [int(x) & 0xFFFFFFFF for x in ks.cpu()]
    assert got == [step + 1, stream_key(seed, step + 1, rank)]


def test_decode_apply_device_step_counter():
    """lr_step derived in the kernel from the device step counter and the device lr (double
    precision, betas as the fp32 kernel arguments) against the host lr_step.

    The bound is on p, and the two lr_steps differ by fp32 roundings (~1e-7 relative), which
    reach p scaled by the step's size: the variances here are at least 1e-4, as after a real
    warm-up, so steps stay below ~0.1 (a step of 4 has an ulp of 5e-7 by itself).  Zero and
    denormal variances are covered bitwise by test_decode_apply_matches_oracle."""
    ops.require()
    N, Tw, t = 2, 6, 19
    lr, b1, b2, eps = 2e-3, 0.9, 0.999, 1e-8
    plan, lay, recv, p0, m0, v0 = _apply_case(N)
    v0 = torch.where(v0 > 0, 1e-4 + 10.0 * v0, v0)
    dp = ops.DevicePlan(plan, DEV)
    rd = recv.to(DEV)
    host = [x.to(DEV) for x in (p0, m0, v0)]
    ops.sign_decode_onebit(dp, rd, lay, *host, 1.0 / N, oracle.onebit_lr_step(lr, b1, b2, t, Tw),
                           eps, b1, b2, Tw)
    dev = [x.to(DEV) for x in (p0, m0, v0)]
    step_t = torch.tensor([t - 1], dtype=torch.int32, device=DEV)
    lr_t = torch.tensor([lr], dtype=torch.float32, device=DEV)
    ops.sign_decode_onebit(dp, rd, lay, *dev, 1.0 / N, 123.0, eps, b1, b2, Tw, step=step_t,
                           lr=77.0, lr_tensor=lr_t)  # lr_step and lr are overridden
    torch.testing.assert_close(dev[0], host[0], rtol=1e-5, atol=1e-6)
    assert not torch.equal(host[0].cpu(), p0)
    assert _bits_equal(dev[1].cpu()[v0 > 0], host[1].cpu()[v0 > 0]) and int(step_t) == t - 1
    dev2 = [x.to(DEV) for x in (p0, m0, v0)]
    ops.sign_decode_onebit(dp, rd, lay, *dev2, 1.0 / N, 123.0, eps, b1, b2, Tw, step=step_t, lr=lr)
    torch.testing.assert_close(dev2[0], host[0], rtol=1e-5, atol=1e-6)


def test_encode_decode_graph_capture():
    """Momentum encode + decode-apply + the step counter's increment captured on one stream and
    replayed with fresh gradients: p, m, the residual and the payload are bitwise the eager run."""
    ops.require()
    plan = _plan([8192 * 2 + 5, 700, 3])
    lay = Layout.build("sign", plan)
    dp = ops.DevicePlan(plan, DEV)
    Tw, b1, b2, eps, wd, lr = 5, 0.9, 0.999, 1e-8, 1e-4, 1e-3
    grads = [_grad(plan, seed=60 + i).to(DEV) for i in range(3)]
    p0 = torch.randn(plan.length, device=DEV)
    v0 = torch.rand(plan.length, device=DEV) * 1e-2
    lr_t = torch.tensor([lr], dtype=torch.float32, device=DEV)

    def state():
        return dict(g=torch.zeros(plan.length, device=DEV), r=torch.zeros(plan.length, device=DEV),
                    p=p0.clone(), m=torch.zeros(plan.length, device=DEV), v=v0.clone(),
                    t=torch.tensor([Tw], dtype=torch.int32, device=DEV),
                    pay=torch.zeros(1, lay.nbytes, dtype=torch.uint8, device=DEV))

    def step(s):
        ops.sign_encode_momentum(dp, s["g"], s["pay"][0], lay, s["r"], s["m"], b1, wd, s["p"])
        ops.sign_decode_onebit(dp, s["pay"], lay, s["p"], s["m"], s["v"], 1.0, 0.0, eps, b1, b2,
                               Tw, step=s["t"], lr=lr, lr_tensor=lr_t)
        s["t"].add_(1)

    eager = state()
    for g in grads:
        eager["g"].copy_(g)
        step(eager)
    cap = state()
    cap["g"].copy_(grads[0])
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        with torch.cuda.graph(graph, stream=side):
            step(cap)
    torch.cuda.current_stream().wait_stream(side)
    graph.replay()  # capturing does not run: this is the first step
    for g in grads[1:]:
        cap["g"].copy_(g)
        graph.replay()
    torch.cuda.synchronize()
    assert int(cap["t"]) == Tw + 3
    for k in ("p", "m", "r", "pay", "v"):
        assert torch.equal(cap[k], eager[k]), k
    assert torch.equal(cap["v"], v0) and not torch.equal(cap["p"], p0)


def test_bad_operands_rejected():
    """Size, dtype, alignment and layout kind are checked on the host, before any launch."""
    ops.require()
    plan = _plan([1000, 8192 + 1])
    lay = Layout.build("sign", plan)
    dp = ops.DevicePlan(plan, DEV)
    g = torch.zeros(plan.length, device=DEV)
    r, m, p, v = (torch.zeros(plan.length, device=DEV) for _ in range(4))
    pay = torch.zeros(lay.nbytes, dtype=torch.uint8, device=DEV)
    big = torch.zeros(plan.length + 4, device=DEV)
    bigpay = torch.zeros(lay.nbytes + 16, dtype=torch.uint8, device=DEV)
    enc = ops.sign_encode_momentum
    with pytest.raises(ValueError):  # no residual / no exp_avg
        enc(dp, g, pay, lay, None, m, 0.9)
    with pytest.raises(ValueError):
        enc(dp, g, pay, lay, r, None, 0.9)
    with pytest.raises(ValueError):  # weight decay without the parameters
        enc(dp, g, pay, lay, r, m, 0.9, 5e-4, None)
    with pytest.raises(ValueError):  # too short
        enc(dp, g, pay[:lay.nbytes - 16], lay, r, m, 0.9)
    with pytest.raises(ValueError):
        enc(dp, g, pay, lay, r, m[:100], 0.9)
    with pytest.raises(ValueError):
        enc(dp, g, pay, lay, r, m, 0.9, 5e-4, p[:100])
    with pytest.raises(TypeError):  # wrong dtypes
        enc(dp, g, pay, lay, r, m.double(), 0.9)
    with pytest.raises(TypeError):
        enc(dp, g, pay, lay, r.to(torch.bfloat16), m, 0.9)
    with pytest.raises(TypeError):
        enc(dp, g, pay, lay, r, m, 0.9, 5e-4, p.half())
    with pytest.raises(ValueError):  # misaligned views
        enc(dp, g, pay, lay, r, big[1:], 0.9)
    with pytest.raises(ValueError):
        enc(dp, g, bigpay[4:], lay, r, m, 0.9)
    with pytest.raises(ValueError):  # another codec's layout
        enc(dp, g, pay, Layout.build("qsgd", plan, 8), r, m, 0.9)
    dec = ops.sign_decode_onebit
    recv = pay[None]
    with pytest.raises(ValueError):  # row length is not the layout's
        dec(dp, bigpay[None], lay, p, m, v, 1.0, 1e-3, 1e-8)
    with pytest.raises(ValueError):  # a missing operand
        dec(dp, recv, lay, p, m, None, 1.0, 1e-3, 1e-8)
    with pytest.raises(ValueError):
        dec(dp, recv, lay, p, m, v[:100], 1.0, 1e-3, 1e-8)
    with pytest.raises(TypeError):
        dec(dp, recv, lay, p, m.double(), v, 1.0, 1e-3, 1e-8)
    with pytest.raises(ValueError):
        dec(dp, recv, lay, big[1:], m, v, 1.0, 1e-3, 1e-8)
    with pytest.raises(ValueError):
        dec(dp, recv, lay, p, m, v, 1.0, 1e-3, 1e-8, freeze_step=0)
    with pytest.raises(TypeError):  # the step counter is int32
        dec(dp, recv, lay, p, m, v, 1.0, 1e-3, 1e-8, step=torch.zeros(1, device=DEV))
    with pytest.raises(ValueError):
        dec(dp, recv, Layout.build("qsgd", plan, 8), p, m, v, 1.0, 1e-3, 1e-8)
    with pytest.raises(TypeError):
        dec(dp, recv, lay, p, m, v, 1.0, 1e-3, 1e-8, shadow=torch.zeros(plan.length, device=DEV))
    torch.cuda.synchronize()
    for t in (pay, g, r, m, p, v):
        assert not t.any()  # nothing ran
