"""PowerSGD's four gfx950 launches (``ops/csrc/powersgd.hip``) against the torch oracle.

One bucket at a non-zero offset of a larger buffer holds the matrix shapes below (those that pass
the compression rule at the tested rank) with three dense tensors mixed in.  Reductions (project,
orthogonalise, back-project, the three-step chain) are compared with the oracle run in fp64: the
kernel's error must be within 3 x the fp32 oracle's own error + 1e-5 (``_rel`` and ``TOL`` of
tests/kernels/test_conv_f32.py; 3 is its allowance for another summation order).  The reconstruct
pass is compared bit for bit."""
import functools

import pytest
import torch

from ewdml import ops
from ewdml.compress import oracle
from tests.powersgd_sim import make_plan, numel, rel, same_bits

pytestmark = pytest.mark.gpu

TOL = 1e-5
RANKS = [1, 2, 4, 8]
MATS = [(20, 25), (10, 500), (50, 500), (64, 64, 3, 3), (513, 1027), (7, 8195), (2048, 9)]
BASE = 128  # the bucket's offset inside the flat buffers
SENTINEL = -77.25
HP = dict(lr=2.0 ** -4, momentum=0.5, dampening=0.0, weight_decay=0.0, nesterov=False)


def _shapes(r):
    keep = [s for s in MATS if numel(s) >= 2 * r * (s[0] + numel(s) // s[0])]
    out = []
    for i, s in enumerate(keep):  # dense tensors between the matrices
        out.append(s)
        if i < 3:
            out.append([(1,), (10,), (500,)][i])
    return out


@functools.lru_cache(maxsize=None)
def _case(r):
    """Plan, inputs (CPU fp32) and the element masks of one rank's bucket."""
    lrp, length = make_plan(_shapes(r), r, bucket_offset=BASE)
    assert len(lrp.dense) == 3 and len(lrp.mats) == len(_shapes(r)) - 3
    # the rule n m >= 2 r (n + m) drops [7, 8195] from rank 4 on (57365 < 65616) and leaves
    # [50, 500], [64, 576] and [513, 1027] at rank 8; [2048, 9] passes up to rank 4
    assert len(lrp.mats) == {1: 7, 2: 7, 4: 6, 8: 3}[r]
    assert ((2048, 9) in lrp.shapes) == (r <= 4)
    assert any(S > 1 for _, S, _, _ in lrp.split) and any(S == 1 for _, S, _, _ in lrp.split)
    gen = torch.Generator().manual_seed(11 + r)
    g = torch.randn(length, generator=gen)
    resid = torch.randn(length, generator=gen) * 0.5
    comp = torch.zeros(length, dtype=torch.bool)
    for off, n, m, *_ in lrp.mats:
        comp[off:off + n * m] = True
    used = comp.clone()
    for off, n_el, *_ in lrp.dense:
        used[off:off + n_el] = True
    resid[~comp] = SENTINEL  # dense tensors and padding keep no residual: never touched
    q = oracle.powersgd_init_q(lrp, 5, 0)
    return lrp, length, g, resid, q, comp, used


def _dev(t, pad=BASE):
    """``t`` as a view at offset ``pad`` of a larger device buffer."""
    buf = torch.full((pad + t.numel() + 64,), SENTINEL, dtype=t.dtype, device="cuda")
    buf[pad:pad + t.numel()] = t.cuda()
    return buf[pad:pad + t.numel()]


def _tables(lrp):
    ops.require()
    return ops.LowRankTables(lrp, "cuda")


def _within(kernel, o32, o64, what):
    ek, eo = rel(kernel, o64), rel(o32, o64)
    print(f"{what}: kernel {ek:.3e}, fp32 oracle {eo:.3e}")
    assert ek <= 3 * eo + TOL, (what, ek, eo)


def _project_all(r):
    lrp, length, g, resid, q, comp, used = _case(r)
    lt = _tables(lrp)
    gd, rd, qd = _dev(g), _dev(resid), _dev(q, 0)
    pd = torch.full((lrp.p_floats + 64,), SENTINEL, device="cuda")
    ops.psgd_project(lt, gd, rd, qd, pd)
    torch.cuda.synchronize()
    return lt, gd, rd, qd, pd


@pytest.mark.parametrize("r", RANKS)
def test_project(r):
    lrp, length, g, resid, q, comp, used = _case(r)
    lt, gd, rd, qd, pd = _project_all(r)
    r32 = resid.clone()
    p32 = oracle.powersgd_project(g, r32, q, lrp)
    r64 = resid.double()
    p64 = oracle.powersgd_project(g.double(), r64, q.double(), lrp, torch.float64)
    nf = lrp.p_factor_floats
    _within(pd[:nf], p32[:nf], p64[:nf], f"P r={r}")
    for _, n, _, po, _, t in lrp.mats:  # and matrix by matrix
        _within(pd[po:po + n * r], p32[po:po + n * r], p64[po:po + n * r], f"P tensor {t}")
    e = rd.cpu()
    assert same_bits(e[comp], (g + resid)[comp]), "stored e is g + residual"
    assert same_bits(e[~comp], resid[~comp]), "dense tensors and padding are untouched"
    assert same_bits(pd[nf:lrp.p_floats], p32[nf:]), "dense tail"
    for off, n_el, tail, _ in lrp.dense:
        assert same_bits(pd[tail:tail + n_el], g[off:off + n_el])
    assert float((pd[lrp.p_floats:] - SENTINEL).abs().max()) == 0.0
    assert same_bits(gd.cpu(), g) and same_bits(qd.cpu(), q)


def _gauss_p(r, zero_col=True):
    lrp = _case(r)[0]
    gen = torch.Generator().manual_seed(23 + r)
    p = torch.randn(lrp.p_floats, generator=gen)
    if zero_col:  # matrix 0 gets an all-zero column
        _, n, _, po, _, _ = lrp.mats[0]
        p[po:po + n * r].view(n, r)[:, min(1, r - 1)] = 0.0
    return lrp, p


@pytest.mark.parametrize("r", RANKS)
def test_orth(r):
    lrp, p = _gauss_p(r)
    lt = _tables(lrp)
    pd = p.cuda()
    ops.psgd_orth(lt, pd, 1.0 / 3)
    p32 = oracle.powersgd_orthogonalize(p.clone(), lrp, 1.0 / 3)
    p64 = oracle.powersgd_orthogonalize(p.double(), lrp, 1.0 / 3, torch.float64)
    out = pd.cpu()
    nf = lrp.p_factor_floats
    _within(out[:nf], p32[:nf], p64[:nf], f"orth r={r}")
    assert same_bits(out[nf:], p[nf:]), "the dense tail is not orthogonalised"
    for i, (_, n, _, po, _, _) in enumerate(lrp.mats):
        P = out[po:po + n * r].view(n, r).double()
        gram = P.t() @ P
        if i == 0:
            c = min(1, r - 1)
            assert bool(torch.isfinite(P).all()) and float(P[:, c].abs().max()) == 0.0
            keep = [k for k in range(r) if k != c]
            gram = gram[keep][:, keep]
            if not keep:
                continue
        assert float((gram - torch.eye(gram.shape[0], dtype=torch.float64)).abs().max()) < 1e-5


def _orth_p(r):
    """An orthonormalised P (fp32 oracle) and the bucket's M for the later launches."""
    lrp, length, g, resid, q, comp, used = _case(r)
    lrp, p = _gauss_p(r, zero_col=False)
    oracle.powersgd_orthogonalize(p, lrp, 1.0)
    M = (g + resid)
    M[~comp] = SENTINEL
    return lrp, p, M


@pytest.mark.parametrize("r", RANKS)
def test_backproject(r):
    lrp, p, M = _orth_p(r)
    lt = _tables(lrp)
    qd = torch.full((lrp.q_floats + 64,), SENTINEL, device="cuda")
    ops.psgd_backproject(lt, _dev(M), p.cuda(), qd)
    q32 = oracle.powersgd_backproject(M, p, lrp)
    q64 = oracle.powersgd_backproject(M.double(), p.double(), lrp, torch.float64)
    _within(qd[:lrp.q_floats], q32, q64, f"Q r={r}")
    for (_, _, m, _, qo, t), (_, S, _, _) in zip(lrp.mats, lrp.split):
        _within(qd[qo:qo + m * r], q32[qo:qo + m * r], q64[qo:qo + m * r],
                f"Q tensor {t} ({S} row splits)")
    assert float((qd[lrp.q_floats:] - SENTINEL).abs().max()) == 0.0
    assert int(lt.tickets.abs().max()) == 0, "the arrival counters are left zeroed"


VARIANTS = [dict(first=True), dict(first=False), dict(first=False, weight_decay=2.0 ** -5),
            dict(first=False, nesterov=True, weight_decay=2.0 ** -5),
            dict(first=True, nesterov=True)]


def _decode_inputs(r):
    lrp, p, M = _orth_p(r)
    length = M.numel()
    gen = torch.Generator().manual_seed(31 + r)
    # dense gradients (summed over "3 ranks") in the tail, a summed Q, parameters and momentum
    p[lrp.p_factor_floats:] = torch.randn(lrp.p_floats - lrp.p_factor_floats, generator=gen)
    q = torch.randn(lrp.q_floats, generator=gen)
    param = torch.randn(length, generator=gen)
    mom = torch.randn(length, generator=gen)
    return lrp, p, M, q, param, mom


@pytest.mark.parametrize("variant", range(len(VARIANTS)))
@pytest.mark.parametrize("r", RANKS)
def test_decode_apply_is_bitwise_the_oracle(r, variant):
    lrp, p, M, q, param, mom = _decode_inputs(r)
    used = _case(r)[6]
    v = dict(VARIANTS[variant])
    first = v.pop("first")
    hp = dict(HP, **v)
    inv_n = 1.0 / 3
    # oracle
    ro, po_, mo = M.clone(), param.clone(), mom.clone()
    go = torch.full_like(M, SENTINEL)
    qa = oracle.powersgd_reconstruct_apply(ro, p, q, lrp, inv_n, po_, mo, hp, first, go)
    # kernel
    lt = _tables(lrp)
    rd, pd, md, gd = _dev(M), _dev(param), _dev(mom), _dev(go * 0 + SENTINEL)
    sh = torch.zeros(M.numel() + BASE, dtype=torch.bfloat16, device="cuda")[BASE:]
    qd, qout = q.cuda(), torch.full((lrp.q_floats + 64,), SENTINEL, device="cuda")
    ops.psgd_decode_apply(lt, rd, p.cuda(), qd, qout, inv_n, param=pd, mom=md, grad_out=gd,
                          lr=hp["lr"], momentum=hp["momentum"], dampening=hp["dampening"],
                          weight_decay=hp["weight_decay"], nesterov=hp["nesterov"], first=first,
                          shadow=sh)
    assert same_bits(gd.cpu(), go), "g^"
    assert same_bits(rd.cpu(), ro), "residual"
    assert same_bits(pd.cpu(), po_), "parameters"
    assert same_bits(md.cpu(), mo), "momentum buffer"
    assert same_bits(qout[:lrp.q_floats], qa), "written-back Q"
    assert float((qout[lrp.q_floats:] - SENTINEL).abs().max()) == 0.0
    assert same_bits(qd.cpu(), q), "the summed Q is only read"
    want_sh = po_.to(torch.bfloat16)
    assert torch.equal(sh.cpu().view(torch.int16)[used], want_sh.view(torch.int16)[used]), "shadow"
    assert float(sh.cpu().float()[~used].abs().max()) == 0.0
    assert not same_bits(pd.cpu(), param)


@pytest.mark.parametrize("r", RANKS)
def test_grad_out_mode_is_bitwise_and_takes_no_step(r):
    lrp, p, M, q, param, mom = _decode_inputs(r)
    ro = M.clone()
    go = torch.full_like(M, SENTINEL)
    qa = oracle.powersgd_reconstruct_apply(ro, p, q, lrp, 0.5, grad_out=go)
    lt = _tables(lrp)
    rd, gd = _dev(M), _dev(go * 0 + SENTINEL)
    qout = torch.zeros(lrp.q_floats, device="cuda")
    ops.psgd_decode_apply(lt, rd, p.cuda(), q.cuda(), qout, 0.5, grad_out=gd)
    assert same_bits(gd.cpu(), go) and same_bits(rd.cpu(), ro) and same_bits(qout, qa)
    with pytest.raises(ValueError):
        ops.psgd_decode_apply(lt, rd, p.cuda(), q.cuda(), qout, 0.5)
    qsame = q.cuda()
    with pytest.raises(ValueError):
        ops.psgd_decode_apply(lt, rd, p.cuda(), qsame, qsame, 0.5, grad_out=gd)


@pytest.mark.parametrize("r", RANKS)
def test_every_launch_is_deterministic(r):
    outs = []
    for _ in range(2):
        lt, gd, rd, qd, pd = _project_all(r)
        lrp = lt.lrp
        first = [pd.clone(), rd.clone()]
        ops.psgd_orth(lt, pd, 1.0 / 3)
        q2 = torch.zeros(lrp.q_floats, device="cuda")
        ops.psgd_backproject(lt, rd, pd, q2)
        qout = torch.zeros(lrp.q_floats, device="cuda")
        param, mom = _dev(_case(r)[2] * 0.25), _dev(_case(r)[2] * 0.5)
        ops.psgd_decode_apply(lt, rd, pd, q2, qout, 1.0 / 3, param=param, mom=mom, lr=0.1,
                              momentum=0.9, first=False)
        outs.append([t.cpu() for t in first + [pd, q2, qout, rd, param, mom]])
    for a, b in zip(*outs):
        assert same_bits(a, b)


def _chain(r, N, steps, kernel, dtype=torch.float32):
    """``steps`` full PowerSGD steps of N simulated ranks (factors summed by hand in rank order)
    through the kernels or through the oracle in ``dtype``; returns (parameters, residuals)."""
    lrp, length, g0, resid0, q0, comp, used = _case(r)
    inv = 1.0 / N
    gen = torch.Generator().manual_seed(41 + r)
    param = torch.randn(length, generator=gen)
    grads = [[torch.randn(length, generator=gen) for _ in range(N)] for _ in range(steps)]
    hp = dict(HP, weight_decay=2.0 ** -5)
    if kernel:
        lt = _tables(lrp)
        pv, mv = _dev(param), _dev(torch.zeros(length))
        resid = [_dev(torch.zeros(length)) for _ in range(N)]
        q = q0.cuda()
        for s in range(steps):
            ps = []
            for k in range(N):
                p = torch.zeros(lrp.p_floats, device="cuda")
                ops.psgd_project(lt, _dev(grads[s][k]), resid[k], q, p)
                ps.append(p)
            p = ps[0].clone()
            for x in ps[1:]:
                p += x
            ops.psgd_orth(lt, p, inv)
            qsum = torch.zeros(lrp.q_floats, device="cuda")
            for k in range(N):
                qk = torch.zeros(lrp.q_floats, device="cuda")
                ops.psgd_backproject(lt, resid[k], p, qk)
                qsum += qk
            qn = torch.zeros(lrp.q_floats, device="cuda")
            for k in range(N):  # every rank reconstructs; rank 0's copy takes the step
                if k == 0:
                    ops.psgd_decode_apply(lt, resid[k], p, qsum, qn, inv, param=pv, mom=mv,
                                          lr=hp["lr"], momentum=hp["momentum"],
                                          weight_decay=hp["weight_decay"], first=s == 0)
                else:
                    scratch = torch.zeros(length, device="cuda")
                    ops.psgd_decode_apply(lt, resid[k], p, qsum, qn, inv, grad_out=scratch)
            q = qn
        return pv.cpu(), torch.stack([x.cpu() for x in resid])
    pv, mv = param.to(dtype), torch.zeros(length, dtype=dtype)
    resid = [torch.zeros(length, dtype=dtype) for _ in range(N)]
    q = q0.to(dtype)
    for s in range(steps):
        ps = [oracle.powersgd_project(grads[s][k].to(dtype), resid[k], q, lrp, dtype)
              for k in range(N)]
        p = ps[0].clone()
        for x in ps[1:]:
            p += x
        oracle.powersgd_orthogonalize(p, lrp, inv, dtype)
        qs = [oracle.powersgd_backproject(resid[k], p, lrp, dtype) for k in range(N)]
        qsum = qs[0].clone()
        for x in qs[1:]:
            qsum += x
        for k in range(N):
            q = oracle.powersgd_reconstruct_apply(resid[k], p, qsum, lrp, inv,
                                                  pv if k == 0 else None, mv if k == 0 else None,
                                                  hp, s == 0, dtype=dtype)
    return pv, torch.stack(resid)


@pytest.mark.parametrize("N", [1, 3])
@pytest.mark.parametrize("r", RANKS)
def test_three_step_chain(r, N):
    comp = _case(r)[5]
    pk, rk = _chain(r, N, 3, True)
    p32, r32 = _chain(r, N, 3, False)
    p64, r64 = _chain(r, N, 3, False, torch.float64)
    _within(pk, p32, p64, f"parameters after 3 steps, r={r}, N={N}")
    _within(rk[:, comp], r32[:, comp], r64[:, comp], f"residual after 3 steps, r={r}, N={N}")
    assert float(rk[:, ~comp].abs().max()) == 0.0
