"""The 8-bit Adam kernel (``ops/csrc/adam8.hip`` through ``ops.adam8_step``) on one MI355X: bitwise
against the torch oracle (``compress/oracle.py adam8_apply``) over three steps, one step from fresh
state against the float64 reference of ``tests/adam8_ref.py``, and the device step counter in a
replayed HIP graph.  Every device buffer is a view 64 elements into a larger allocation whose other
bytes hold 0x5A, as do the code arrays' pads between tensors; all must be unchanged afterwards."""
import functools

import pytest
import torch

from ewdml import ops
from ewdml.compress import oracle
from ewdml.compress.plan import BucketPlan
from tests import adam8_ref as A
from tests import optim_ref as R

pytestmark = pytest.mark.gpu

GUARD, PAT = 64, 0x5A
DT = {"fp32": torch.float32, "bf16": torch.bfloat16, "fp16": torch.float16}
BETAS = (A.HP["beta1"], A.HP["beta2"])


class Buf:
    def __init__(self, values):
        n, self.g = values.numel(), GUARD * values.element_size()
        self.raw = torch.full((self.g * 2 + n * values.element_size(),), PAT, dtype=torch.uint8,
                              device="cuda")
        self.v = self.raw.view(values.dtype)[GUARD:GUARD + n]
        self.v.copy_(values)

    def guards_ok(self):
        r = self.raw.cpu()
        return bool((r[:self.g] == PAT).all() and (r[-self.g:] == PAT).all())


def _bits(t):
    return t.cpu().contiguous().view(torch.uint8)


def _state(name):
    length, _, chunks, pad = A.layout(A.RANGES[name])
    st = list(oracle.adam8_state(length, chunks))
    st[0][pad] = st[1][pad] = PAT
    return st


def _plan(name, am, av):
    length, blocks, _, _ = A.layout(A.RANGES[name])
    return ops.Adam8Plan(BucketPlan(A.RANGES[name], [b[0] for b in blocks], 1.0, 0, length), am, av)


@functools.lru_cache(maxsize=None)
def _oracle(name, gdt, wd, steps):
    blocks = A.layout(A.RANGES[name])[1]
    p0, grads = A.inputs(name, steps, DT[gdt])
    p, st = p0.clone(), _state(name)
    for t, g in enumerate(grads, 1):
        oracle.adam8_apply(p, *st, g.float(), blocks, A.HP["lr"], *BETAS, A.HP["eps"], wd, t)
    return p0, grads, p, st


@pytest.mark.parametrize("wd", [0.0, 1e-2])
@pytest.mark.parametrize("gdt", list(DT))
@pytest.mark.parametrize("name", list(A.RANGES))
def test_kernel_is_the_oracle_bitwise(name, gdt, wd):
    ops.require()
    p0, grads, p_or, st_or = _oracle(name, gdt, wd, 3)
    _, blocks, _, pad = A.layout(A.RANGES[name])
    bufs = [Buf(p0)] + [Buf(x) for x in _state(name)] + [Buf(torch.zeros_like(p0, dtype=DT["bf16"]))]
    p, cm, cv, am, av, sh = bufs
    sh.v.view(torch.uint8).fill_(PAT)
    plan, gs = _plan(name, am.v, av.v), [Buf(g) for g in grads]
    for t, g in enumerate(gs, 1):
        ops.adam8_step(plan, p.v, g.v, cm.v, cv.v, eps=A.HP["eps"], betas=BETAS, weight_decay=wd,
                       lr_step=oracle.adam8_lr_step(A.HP["lr"], *BETAS, t), shadow=sh.v)
    torch.cuda.synchronize()
    want_sh = torch.where(pad, torch.full((), PAT * 257, dtype=torch.int16).view(DT["bf16"]),
                          p_or.to(DT["bf16"]))
    for nm, got, want in zip(("param", "code_m", "code_v", "absmax_m", "absmax_v", "shadow"), bufs,
                             [p_or] + st_or + [want_sh]):
        assert torch.equal(_bits(got.v), _bits(want)), nm
        assert got.guards_ok(), f"{nm}: guard bytes were written"
    assert gs[0].guards_ok()


@pytest.mark.parametrize("wd", [0.0, 1e-2])
def test_first_step_against_float64(wd):
    """Near a midpoint (``x`` within relative 2^-18 of it in float64) a code may differ by one;
    such elements must stay under 0.5 % of the range.  Observed on these inputs: 0.011 % (with
    weight decay 0.022 %) of the first-moment and 0.011 % of the second-moment elements, and no
    code differing at all, for the CPU oracle and the kernel alike."""
    ops.require()
    length, blocks, chunks, pad = A.layout(A.RANGES["all"])
    live = ~pad
    p0, (g,) = A.inputs("all", 1)
    p64, st64 = p0.double(), A.fresh(length, chunks)
    near = A.step64(p64, *st64, g, blocks, 1, weight_decay=wd, **A.HP)
    p32, m32, v32 = p0.clone(), torch.zeros(length), torch.zeros(length)
    R.adam32(p32, m32, v32, None, g, R.lr_step64(A.HP["lr"], *BETAS, 1), beta1=BETAS[0],
             beta2=BETAS[1], eps=A.HP["eps"], weight_decay=wd)
    p_or, st_or = _oracle("all", "fp32", wd, 1)[2:]
    p, cm, cv, am, av = [Buf(p0)] + [Buf(x) for x in _state("all")]
    ops.adam8_step(_plan("all", am.v, av.v), p.v, Buf(g).v, cm.v, cv.v, eps=A.HP["eps"],
                   betas=BETAS, weight_decay=wd, lr_step=oracle.adam8_lr_step(A.HP["lr"], *BETAS, 1))
    torch.cuda.synchronize()
    R.check("param", p.v.cpu()[live], p32[live], p64[live], f"wd {wd} ")
    for nm, got, x32, x64 in (("absmax_m", am, m32.abs(), st64[2]), ("absmax_v", av, v32, st64[3])):
        ref32 = torch.zeros(x64.numel())  # the CPU fp32 reference's block maxima
        for o, n, s0 in blocks:
            for j in range((n + A.BLOCK - 1) // A.BLOCK):
                ref32[s0 + j] = x32[o + A.BLOCK * j:o + min(n, A.BLOCK * (j + 1))].max()
        R.check(nm, got.v.cpu(), ref32, x64, f"wd {wd} ")
    for i, nm in enumerate(("code_m", "code_v")):
        nr = near[i][live]
        print(f"wd {wd} {nm}: near a midpoint {100 * float(nr.float().mean()):.4f} %")
        assert float(nr.float().mean()) <= 0.005
        for who, c in (("oracle", st_or[i]), ("kernel", (cm, cv)[i].v.cpu())):
            d = (c.long() - st64[i])[live].abs()
            print(f"  {who}: {int((d != 0).sum())} codes differ")
            assert bool((d[~nr] == 0).all()) and int(d.max()) <= 1, f"{nm} ({who})"


def test_device_counter_in_a_replayed_graph():
    """One captured launch replayed five times against five eager launches, device step counter
    and lr: codes and absmax bitwise, parameters against float64 within ``optim_ref.limit`` (the
    device's ``pow`` is not correctly rounded: test_optim_hip.py's contract for k_adam_flat)."""
    ops.require()
    steps, wd = 5, 1e-2
    length, blocks, chunks, _ = A.layout(A.RANGES["all"])
    p0, grads, p_or, _ = _oracle("all", "fp32", wd, steps)
    p64, st64 = p0.double(), A.fresh(length, chunks)
    for t, g in enumerate(grads, 1):
        A.step64(p64, *st64, g, blocks, t, weight_decay=wd, **A.HP)
    lr_t = torch.full((1,), A.HP["lr"], dtype=torch.float32, device="cuda")
    runs = []
    for graphed in (False, True):
        bufs = [Buf(p0)] + [Buf(x) for x in _state("all")] + [Buf(grads[0])]
        p, cm, cv, am, av, gbuf = bufs
        plan = _plan("all", am.v, av.v)
        step_t = torch.zeros(1, dtype=torch.int32, device="cuda")

        def launch():
            ops.adam8_step(plan, p.v, gbuf.v, cm.v, cv.v, eps=A.HP["eps"], betas=BETAS,
                           weight_decay=wd, step=step_t, lr=123.0, lr_tensor=lr_t)
            step_t.add_(1)

        graph = torch.cuda.CUDAGraph()
        if graphed:
            with torch.cuda.graph(graph):
                launch()
        for g in grads:
            gbuf.v.copy_(g)
            graph.replay() if graphed else launch()
        torch.cuda.synchronize()
        assert int(step_t.item()) == steps and all(b.guards_ok() for b in bufs)
        runs.append([x.v.cpu() for x in bufs[:5]])
    for a, b in zip(*runs):
        assert torch.equal(_bits(a), _bits(b))
    R.check("param", runs[1][0], p_or, p64, "graph ")
