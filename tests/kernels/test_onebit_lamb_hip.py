"""1-bit LAMB's HIP kernels (ops/csrc/sign_codec.hip: k_sign_decode_lamb_stage and
k_lamb_onebit_apply) vs the torch oracle, on one MI355X.

Exactness contract: with bc1 passed from the host, the parameters, the averaged momentum, the
fresh variance, the per-tensor factors and the ratios are bitwise ``oracle.onebit_lamb_apply``'s:
every operation is rounded separately on both sides, sqrtf and the divides are IEEE, the file set
is built with -ffp-contract=off, and a maximum does not depend on its order.
"""
import pytest
import torch

from ewdml import ops
from ewdml.compress import oracle
from ewdml.compress.plan import BucketPlan, Layout
from ewdml.compress.rng import stream_key

pytestmark = pytest.mark.gpu

DEV = "cuda"
SHAPES = [[10], [1, 2, 3, 4, 5], [500, 10], [8192 * 3 + 5, 7, 64, 100003]]
B1, B2, EPS, TW = 0.9, 0.999, 1e-8, 4


def _plan(numels, bucket_offset=4096):
    offs, o = [], 0
    for n in numels:
        offs.append(o)
        o += (n + 63) // 64 * 64
    return BucketPlan(numels, offs, 1.0, bucket_offset, o)


def _rand(plan, seed, scale=1.0):
    g = torch.zeros(plan.length)
    gen = torch.Generator().manual_seed(seed)
    for off, n in zip(plan.offsets, plan.numels):
        g[off:off + n] = torch.randn(n, generator=gen) * scale * (0.1 + torch.rand(1, generator=gen))
    return g


def _bits(a, b):
    return torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def _payloads(plan, lay, N, seed):
    # very different magnitudes per rank: the rank order of the fp32 sum matters
    return torch.stack([oracle.encode_sign(_rand(plan, seed + r) * (3.0 ** r), plan, lay)
                        for r in range(N)])


class Case:
    """Host state of one bucket and its device twin."""

    def __init__(self, numels, seed=0, adapt=None):
        self.plan = plan = _plan(numels)
        self.lay = Layout.build("sign", plan)
        T = plan.num_tensors
        gen = torch.Generator().manual_seed(seed)
        self.p = torch.randn(plan.length, generator=gen)
        self.m = torch.randn(plan.length, generator=gen) * 0.05
        self.v = torch.rand(plan.length, generator=gen) * 1e-2 + 1e-4
        self.v[::5] = 0.0  # coordinates that never saw a gradient
        self.v[3::7] = 1e-42  # denormal variances take the step
        self.vf = torch.rand(plan.length, generator=gen) * 1e-2 + 1e-4
        self.adapt = [(t % 3 != 1) for t in range(T)] if adapt is None else adapt
        self.tensors = [(o, n, a) for o, n, a in zip(plan.offsets, plan.numels, self.adapt)]
        self.r_frozen = torch.rand(T, generator=gen) + 0.5
        self.factors = torch.ones(2, T)
        self.ratio = torch.full((T,), -1.0)
        self.inside = torch.zeros(plan.length, dtype=torch.bool)
        for o, n in zip(plan.offsets, plan.numels):
            self.inside[o:o + n] = True

    def device(self):
        d = type("Dev", (), {})()
        d.dp = ops.DevicePlan(self.plan, DEV)
        for k in ("p", "m", "v", "vf", "r_frozen", "factors", "ratio"):
            setattr(d, k, getattr(self, k).clone().to(DEV))
        d.adapt = torch.tensor(self.adapt, dtype=torch.int32, device=DEV)
        d.partials = torch.full((self.plan.num_chunks,), float("nan"), device=DEV)
        d.shadow = torch.zeros(self.plan.length, dtype=torch.bfloat16, device=DEV)
        d.lt = ops.OnebitLambTables(d.dp, d.adapt, d.r_frozen, d.factors, d.ratio, d.partials)
        return d

    def host_step(self, recv, t, lr, wd, inv_n):
        ratios, fac = oracle.onebit_lamb_apply(
            recv, self.plan, self.lay, self.p, self.m, self.v, self.vf, self.tensors,
            self.r_frozen, self.factors[(t - 1) & 1], inv_n, lr, B1, B2, EPS, wd, t, TW)
        self.ratio.copy_(ratios)
        self.factors[t & 1] = fac

    def dev_step(self, d, recv, t, lr, wd, inv_n, **kw):
        ops.onebit_lamb_step(d.lt, recv, self.lay, d.p, d.m, d.v, d.vf, inv_n, lr=lr,
                             betas=(B1, B2), eps=EPS, weight_decay=wd, t=t, freeze_step=TW,
                             bc1=1.0 - B1 ** t, shadow=d.shadow, **kw)

    def compare(self, d, what=""):
        for k in ("p", "m", "vf", "v", "ratio", "factors"):
            got, ref = getattr(d, k).cpu(), getattr(self, k)
            if got.shape == self.inside.shape:
                assert _bits(got[self.inside], ref[self.inside]), f"{what}: {k}"
                assert _bits(got[~self.inside], ref[~self.inside]), f"{what}: {k} between tensors"
            else:
                assert _bits(got, ref), f"{what}: {k} {got} vs {ref}"


@pytest.mark.parametrize("N", [1, 2, 3, 8])
@pytest.mark.parametrize("numels", SHAPES)
def test_stage_and_apply_match_oracle(numels, N):
    """Two consecutive steps (the second reads the factors the first wrote into the other row),
    weight decay on and off, the bf16 shadow and the RNG key advance."""
    ops.require()
    c = Case(numels, seed=len(numels) + N)
    d = c.device()
    v0 = c.v.clone()
    seed, step0, rank = 5, 41, 3
    ks = torch.tensor([step0, 0], dtype=torch.int32, device=DEV)
    for i, (t, wd) in enumerate(((TW + 1, 5e-4), (TW + 2, 0.0))):
        recv = _payloads(c.plan, c.lay, N, seed=100 + 10 * i)
        c.host_step(recv, t, 2e-3, wd, 1.0 / N)
        c.dev_step(d, recv.to(DEV), t, 2e-3, wd, 1.0 / N, key_state=ks, key_seed=seed,
                   key_rank=rank)
        c.compare(d, f"step {t}")
        m_ref = oracle.decode_sum(recv, c.plan, c.lay, 0, 1.0 / N)
        assert _bits(d.m.cpu()[c.inside], m_ref[c.inside])
        for o, n in zip(c.plan.offsets, c.plan.numels):
            assert torch.equal(d.shadow[o:o + n], d.p[o:o + n].to(torch.bfloat16))
    assert _bits(d.v.cpu(), v0)  # the frozen variance is only read
    still = c.inside & (v0 == 0)
    assert bool((d.m.cpu()[still] != 0).all())
    got = [int(x) & 0xFFFFFFFF for x in ks.cpu()]
    assert got == [step0 + 2, stream_key(seed, step0 + 2, rank)]
    # both factor rows were written, and the adapting tensors moved off 1
    ad = torch.tensor(c.adapt)
    assert bool((c.factors[:, ~ad] == 1).all()) and bool((c.factors[:, ad] != 1).any())
    assert bool((c.ratio[~ad] == 1).all())


def test_maximum_placement():
    """The tensor's largest q planted in its last chunk, in the scalar tail of its last chunk and
    in its first chunk; one tensor whose v is 0 everywhere; one NaN in the fresh variance.

    Every other coordinate has q in [0.91, 0.95] and the planted one 1.05, inside the last
    factor's band [0.9, 1.1]: the factor is the planted q itself, unclipped."""
    ops.require()
    numels = [8192 * 2 + 5, 8192 * 3 + 102, 8192 + 40, 64, 5000]
    c = Case(numels, seed=9, adapt=[True] * 5)
    N, t = 1, TW + 1
    recv = _payloads(c.plan, c.lay, N, seed=7)
    c.m.zero_()
    c.vf.fill_(1.0)
    probe = Case(numels, seed=9, adapt=[True] * 5)  # the fresh variance this step will store
    probe.m.zero_()
    probe.vf.fill_(1.0)
    probe.host_step(recv, t, 1e-3, 0.0, 1.0)
    gen = torch.Generator().manual_seed(1)
    k = 0.91 + 0.04 * torch.rand(c.plan.length, generator=gen)
    o = c.plan.offsets
    # tensor 0: its last chunk; tensor 1: the last element (its last chunk holds 102 elements, 100
    # in 16-byte groups and 2 in the scalar tail); tensor 2: its first chunk
    for s in (o[0] + 8192 * 2 + 1, o[1] + numels[1] - 1, o[2] + 17):
        k[s] = 1.05
    c.v = (k * probe.vf.double().sqrt().float()) ** 2
    c.v[o[3]:o[3] + 64] = 0.0
    c.vf[o[4] + 4321] = float("nan")
    c.factors[0, 3] = 1.3  # the factor an all-zero tensor must keep
    d = c.device()
    c.host_step(recv, t, 1e-3, 0.0, 1.0)
    c.dev_step(d, recv.to(DEV), t, 1e-3, 0.0, 1.0)
    c.compare(d, "planted")
    f = c.factors[t & 1]
    assert all(1.04 < float(f[i]) < 1.06 for i in range(3)), f
    assert float(f[3]) == float(c.factors[0, 3]) and float(c.ratio[3]) == float(c.r_frozen[3])
    assert 0.9 <= float(f[4]) < 0.96 and torch.isnan(d.vf[o[4] + 4321])
    parts = d.partials.cpu()
    assert not torch.isnan(parts).any() and parts.numel() == c.plan.num_chunks


def test_run_to_run_identical():
    ops.require()
    c = Case(SHAPES[3], seed=2)
    recv = _payloads(c.plan, c.lay, 3, seed=50).to(DEV)
    outs = []
    for _ in range(2):
        d = c.device()
        c.dev_step(d, recv, TW + 3, 1e-3, 1e-4, 1.0 / 3)
        outs.append(d)
    for k in ("p", "m", "vf", "ratio", "factors", "partials", "shadow"):
        a, b = getattr(outs[0], k), getattr(outs[1], k)
        assert torch.equal(a.view(torch.int16) if a.dtype == torch.bfloat16 else
                           a.view(torch.int32),
                           b.view(torch.int16) if b.dtype == torch.bfloat16 else
                           b.view(torch.int32)), k


def test_graph_replays_follow_the_device_lr_and_step():
    """Momentum encode + stage + apply + the step counter's increment captured once and replayed
    three times with the lr changed in between: bitwise three eager steps that read the same
    device scalars.  Against steps whose t, bc1 and lr come from the host the parameters get
    the bound test_onebit_adam_hip.py gives 1-bit Adam's device-derived lr_step (the derived
    scalars differ by fp32 roundings, which reach p scaled by the step's size); the momentum and
    the fresh variance, which depend on neither, stay bitwise."""
    ops.require()
    c = Case([8192 * 2 + 5, 700, 3], seed=3, adapt=[True, True, False])
    c.v = torch.where(c.v > 0, 1e-4 + 10.0 * c.v, c.v)  # as after a real warm-up: steps < ~0.1
    plan, lay = c.plan, c.lay
    grads = [_rand(plan, 60 + i).to(DEV) for i in range(3)]
    lrs = [2e-3, 1e-3, 2.5e-4]
    wd = 1e-4

    def state():
        d = c.device()
        d.g = torch.zeros(plan.length, device=DEV)
        d.r = torch.zeros(plan.length, device=DEV)
        d.t = torch.tensor([TW], dtype=torch.int32, device=DEV)
        d.lr = torch.tensor([lrs[0]], dtype=torch.float32, device=DEV)
        d.pay = torch.zeros(1, lay.nbytes, dtype=torch.uint8, device=DEV)
        return d

    def step(d, host_t=None, host_lr=None):
        ops.sign_encode_momentum(d.dp, d.g, d.pay[0], lay, d.r, d.m, B1, 0.0, d.p)
        if host_t is None:
            c.dev_step(d, d.pay, 1, 77.0, wd, 1.0, step=d.t, lr_tensor=d.lr)  # t, lr overridden
        else:
            c.dev_step(d, d.pay, host_t, host_lr, wd, 1.0)
        d.t.add_(1)

    eager, host = state(), state()
    for i, g in enumerate(grads):
        for d in (eager, host):
            d.g.copy_(g)
        eager.lr.fill_(lrs[i])
        step(eager)
        step(host, TW + 1 + i, lrs[i])
    cap = state()
    cap.g.copy_(grads[0])
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        with torch.cuda.graph(graph, stream=side):
            step(cap)
    torch.cuda.current_stream().wait_stream(side)
    graph.replay()  # capturing does not run: this is the first step
    for i in (1, 2):
        cap.g.copy_(grads[i])
        cap.lr.fill_(lrs[i])
        graph.replay()
    torch.cuda.synchronize()
    assert int(cap.t) == TW + 3
    for k in ("p", "m", "vf", "v", "r", "pay", "ratio", "factors", "shadow"):
        assert torch.equal(getattr(cap, k), getattr(eager, k)), k
    assert not torch.equal(cap.p, c.p.to(DEV)) and _bits(cap.v.cpu(), c.v)
    torch.testing.assert_close(eager.p, host.p, rtol=1e-5, atol=1e-6)
    for k in ("m", "vf", "factors"):
        assert _bits(getattr(eager, k).cpu(), getattr(host, k).cpu()), k
    torch.testing.assert_close(eager.ratio, host.ratio, rtol=0, atol=0)


def test_two_launches_per_bucket(monkeypatch):
    C = ops.require()
    c = Case([8192 + 9, 300], seed=1)
    d = c.device()
    recv = _payloads(c.plan, c.lay, 2, seed=3).to(DEV)
    calls = []
    for op, name in enumerate(("sign_decode_lamb_stage", "lamb_onebit_apply")):
        real = getattr(C, name)
        monkeypatch.setattr(ops._C, name,
                            lambda a, op=op, real=real: (calls.append(op), real(a))[1])
    c.dev_step(d, recv, TW + 1, 1e-3, 0.0, 0.5)
    assert calls == [0, 1]
    monkeypatch.undo()
    torch.cuda.synchronize()
    gr = torch.cuda.CUDAGraph(keep_graph=True)
    with torch.cuda.graph(gr, capture_error_mode="thread_local"):
        c.dev_step(d, recv, TW + 2, 1e-3, 0.0, 0.5)
    info = ops.graph_info(gr.raw_cuda_graph())
    assert info["linear"] and info["types"] == {"kernel": 2}, info


def test_bad_operands_rejected():
    """Size, dtype, alignment, rank count and layout kind are checked on the host, before any
    launch."""
    ops.require()
    c = Case([1000, 8192 + 1], seed=0)
    plan, lay = c.plan, c.lay
    d = c.device()
    for k in ("p", "m", "v", "vf"):
        getattr(d, k).zero_()
    pay = torch.zeros(1, lay.nbytes, dtype=torch.uint8, device=DEV)
    big = torch.zeros(plan.length + 4, device=DEV)
    bigpay = torch.zeros(lay.nbytes + 16, dtype=torch.uint8, device=DEV)

    def run(recv=pay, p=d.p, m=d.m, v=d.v, vf=d.vf, layout=lay, t=TW + 1, **kw):
        args = dict(lr=1e-3, t=t, freeze_step=TW)
        args.update(kw)
        ops.onebit_lamb_step(d.lt, recv, layout, p, m, v, vf, 1.0, **args)

    with pytest.raises(ValueError):  # a short recv / a row that is not the layout's
        run(recv=pay[:, :lay.nbytes - 16])
    with pytest.raises(ValueError):
        run(recv=bigpay[None])
    with pytest.raises(ValueError):  # nranks = 0
        run(recv=pay[:0])
    with pytest.raises(ValueError):  # misaligned pointers
        run(p=big[1:])
    with pytest.raises(ValueError):
        run(vf=big[1:])
    with pytest.raises(ValueError):
        run(recv=bigpay[4:4 + lay.nbytes][None])
    with pytest.raises(ValueError):  # a missing or short operand
        run(vf=None)
    with pytest.raises(ValueError):
        run(v=d.v[:100])
    with pytest.raises(TypeError):
        run(m=d.m.double())
    with pytest.raises(ValueError):  # not a compressed-stage step
        run(t=TW)
    with pytest.raises(ValueError):
        run(freeze_step=0)
    with pytest.raises(TypeError):  # the step counter is int32
        run(step=torch.zeros(1, device=DEV))
    with pytest.raises(ValueError):  # another codec's layout
        run(layout=Layout.build("qsgd", plan, 8))
    with pytest.raises(TypeError):
        run(shadow=torch.zeros(plan.length, device=DEV))
    T = plan.num_tensors
    with pytest.raises(ValueError):  # tables of another size
        ops.OnebitLambTables(d.dp, d.adapt, d.r_frozen, torch.ones(2, T + 1, device=DEV), d.ratio,
                             d.partials)
    with pytest.raises(ValueError):
        ops.OnebitLambTables(d.dp, d.adapt, d.r_frozen, d.factors, d.ratio, d.partials[:-1])
    with pytest.raises(TypeError):
        ops.OnebitLambTables(d.dp, d.adapt.float(), d.r_frozen, d.factors, d.ratio, d.partials)
    torch.cuda.synchronize()
    for x in (d.p, d.m, d.v, d.vf):
        assert not x.any()  # nothing ran
    assert torch.isnan(d.partials).all() and bool((d.ratio == -1).all())
