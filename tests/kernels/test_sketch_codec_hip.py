"""The count sketch's gfx950 launches (``ops/csrc/sketch_codec.hip``) against the torch oracle, bit
for bit: stage, table (both widths, 1 / 3 / 5 rows, the hand-set wrap and no-wrap shifts, more
chunks than one summation group; twice, so no order depends on scheduling), estimate (from a
table pre-summed over two ranks), select + gather (index lists, and a bitmap-indexed tensor at
ratio 0.25) and the apply through the plain top-k decode (SGD with momentum at a first and a later
step, ``grad_out``, the bf16 shadow, 1 / N for N = 1, 2, 3).

Every device operand is a view inside a larger sentinel-filled buffer, checked after each launch."""
import functools

import pytest
import torch

from ewdml import ops
from ewdml.compress import oracle
from tests import sketch_sim as S

pytestmark = pytest.mark.gpu

PAD = 128
SENTINEL = -77.25
HP = dict(lr=2.0 ** -4, momentum=0.5, dampening=0.0, weight_decay=0.0, nesterov=False)
CASES = [(r, w) for r in (1, 3, 5) for w in (1.0, 2.0)]
BITMAP = dict(numels=S.NUMELS[:4], ratio=0.25)  # tensor 0: k = 6148 of 24593, bitmap-indexed


class _Dev:
    """A CPU tensor as a view at offset PAD of a sentinel-filled device buffer."""

    def __init__(self, t):
        fill = SENTINEL if t.dtype.is_floating_point else 0x5A
        self.buf = torch.full((PAD + t.numel() + PAD,), fill, dtype=t.dtype, device="cuda")
        self.v = self.buf[PAD:PAD + t.numel()]
        self.v.copy_(t)
        self.fill = self.buf[0].clone()  # the sentinel as this dtype holds it

    def intact(self):
        n = self.v.numel()
        return bool((self.buf[:PAD] == self.fill).all() and (self.buf[PAD + n:] == self.fill).all())


@functools.lru_cache(maxsize=None)
def _case(rows, width, bitmap=False):
    """Plans, inputs and every oracle result of one case (CPU, computed once)."""
    sp, lay, _ = S.make_plans(rows, width, **(BITMAP if bitmap else {}))
    L = sp.plan.length
    gen = torch.Generator().manual_seed(17 + rows)
    g = [torch.randn(L, generator=gen) for _ in range(2)]
    for x in g:
        x[torch.randperm(L, generator=gen)[:L // 40]] *= 25.0
    resid0 = [torch.randn(L, generator=gen) * 0.5 for _ in range(2)]
    keep = torch.zeros(L, dtype=torch.bool)
    for t in sp.sketched:
        keep[sp.plan.offsets[t]:sp.plan.offsets[t] + sp.plan.numels[t]] = True
    for r in resid0:
        r[~keep] = 0.0  # dense tensors and pads keep no residual
    acc = [r.clone() for r in resid0]
    for x, a in zip(g, acc):
        oracle.sketch_stage(x, a, sp)
    tables = [oracle.sketch_accumulate(a, sp) for a in acc]
    T = tables[0] + tables[1]
    est = oracle.sketch_estimate(T, sp)
    resid1 = acc[0].clone()
    pay = oracle.sketch_select(est, sp, lay)
    pay_est = pay.clone()
    oracle.sketch_gather(pay, g[0], resid1, sp, lay)
    return dict(sp=sp, lay=lay, L=L, g=g, resid0=resid0, acc=acc, tables=tables, T=T, est=est,
                pay_est=pay_est, pay=pay, resid1=resid1)


@functools.lru_cache(maxsize=None)
def _tables(rows, width, bitmap=False):
    ops.require()
    c = _case(rows, width, bitmap)
    return ops.SketchTables(c["sp"], "cuda"), ops.DevicePlan(c["sp"].plan, "cuda")


def test_plans_cover_the_edges():
    c = _case(3, 2.0)
    sp = c["sp"]
    assert sp.plan.num_chunks > ops.SKETCH_SUM_GROUP and sp.shifts[0][0] == sp.W - 1
    assert sp.shifts[0][3] == sp.W - 17 and sp.chunk_rows[3][1] == 17
    assert sp.dense == [False, False, True, True, False]
    b = _case(3, 2.0, True)["sp"].plan
    assert b.tensor_bm0[0] >= 0 and b.tensor_idx0[3] >= 0  # bitmap tensors and an index list
    assert all(i >= 0 for i in sp.plan.tensor_idx0[:2])  # index lists at ratio 0.01


@pytest.mark.parametrize("rows,width", CASES[:2])
def test_stage(rows, width):
    c = _case(rows, width)
    st, _ = _tables(rows, width)
    g, resid = _Dev(c["g"][0]), _Dev(c["resid0"][0])
    ops.sketch_stage(st, g.v, resid.v)
    torch.cuda.synchronize()
    assert S.same_bits(resid.v, c["acc"][0]) and resid.intact()
    assert S.same_bits(g.v, c["g"][0])


@pytest.mark.parametrize("rows,width", CASES)
def test_table_is_the_oracles_and_the_same_twice(rows, width):
    c = _case(rows, width)
    st, _ = _tables(rows, width)
    acc = _Dev(c["acc"][0])
    out = []
    for _ in range(2):
        table = _Dev(torch.full((c["sp"].table_floats,), 3.0))  # every entry is overwritten
        ops.sketch_accum(st, acc.v, table.v)
        torch.cuda.synchronize()
        assert table.intact()
        out.append(table.v.clone())
    assert S.same_bits(out[0], out[1])
    assert S.same_bits(out[0], c["tables"][0])


@pytest.mark.parametrize("rows,width", CASES)
def test_estimate_from_a_summed_table(rows, width):
    c = _case(rows, width)
    st, _ = _tables(rows, width)
    table, est = _Dev(c["T"]), _Dev(torch.zeros(c["L"]))
    ops.sketch_estimate(st, table.v, est.v)
    torch.cuda.synchronize()
    assert S.same_bits(est.v, c["est"]) and est.intact()


@pytest.mark.parametrize("rows,width,bitmap", [(3, 2.0, False), (1, 1.0, False), (3, 2.0, True)])
def test_select_and_gather(rows, width, bitmap):
    c = _case(rows, width, bitmap)
    st, dp = _tables(rows, width, bitmap)
    lay = c["lay"]
    est, g, resid = _Dev(c["est"]), _Dev(c["g"][0]), _Dev(c["acc"][0])
    pay = _Dev(torch.zeros(lay.nbytes, dtype=torch.uint8))
    ops.topk_encode(dp, est.v, pay.v, lay, 127, "max", 0, predict=False)
    torch.cuda.synchronize()
    assert torch.equal(pay.v.cpu(), c["pay_est"]), "the exact top-k passes select as the oracle"
    ops.sketch_gather(st, dp, pay.v, lay, g.v, resid.v)
    torch.cuda.synchronize()
    assert torch.equal(pay.v.cpu(), c["pay"]), "values"
    assert S.same_bits(resid.v, c["resid1"]), "zeroed residual"
    assert pay.intact() and resid.intact() and S.same_bits(g.v, c["g"][0])


def _apply_ref(c, n, first, param, mom):
    sp, lay = c["sp"], c["lay"]
    ghat = oracle.decode_sum(c["pay"][None], sp.plan, lay, 127, 1.0 / n)
    for off, ln in zip(sp.plan.offsets, sp.plan.numels):
        oracle.sgd_apply(param[off:off + ln], mom[off:off + ln], ghat[off:off + ln], HP["lr"],
                         HP["momentum"], 0.0, 0.0, False, first)
    return ghat


@pytest.mark.parametrize("bitmap", [False, True])
@pytest.mark.parametrize("n", [1, 2, 3])
def test_apply_is_the_plain_topk_decode_of_the_summed_payload(n, bitmap):
    c = _case(3, 2.0, bitmap)
    _, dp = _tables(3, 2.0, bitmap)
    lay, L = c["lay"], c["L"]
    gen = torch.Generator().manual_seed(23)
    p_ref, m_ref = torch.randn(L, generator=gen), torch.zeros(L)
    param, mom = _Dev(p_ref), _Dev(m_ref)
    shadow, gout = _Dev(p_ref.to(torch.bfloat16)), _Dev(torch.zeros(L))
    pay = _Dev(c["pay"])
    for first in (True, False):  # the momentum buffer is written, then read
        ghat = _apply_ref(c, n, first, p_ref, m_ref)
        ops.topk_decode_apply(dp, pay.v.unsqueeze(0), lay, 127, param=param.v, mom=mom.v,
                              grad_out=gout.v, grad_scale=1.0 / n, first=first, shadow=shadow.v,
                              **{k: HP[k] for k in ("lr", "momentum")})
        torch.cuda.synchronize()
        assert S.same_bits(gout.v, ghat), ("grad_out", first)
        assert S.same_bits(param.v, p_ref) and S.same_bits(mom.v, m_ref), first
        used = torch.zeros(L, dtype=torch.bool)
        for off, ln in zip(c["sp"].plan.offsets, c["sp"].plan.numels):
            used[off:off + ln] = True
        assert torch.equal(shadow.v.cpu()[used], p_ref.to(torch.bfloat16)[used]), first
    assert all(d.intact() for d in (param, mom, shadow, gout, pay))
