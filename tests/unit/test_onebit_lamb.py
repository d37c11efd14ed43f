"""1-bit LAMB on the CPU: the receive side of the torch oracle (compress/oracle.py
``onebit_lamb_apply``), ``FlatOnebitLamb`` (optim/flat.py), the trainer's stage switch in a world
of one, and the command line."""
import math

import numpy as np
import pytest
import torch

import ewdml
from ewdml.compress import oracle
from ewdml.compress.plan import BucketPlan, Layout

F = np.float32
BASE = ["--network", "LeNet", "--dataset", "MNIST", "--batch-size", "16", "--synthetic-size",
        "256", "--eval-freq", "0", "--quiet", "--device", "cpu", "--lr", "0.001",
        "--log-interval", "1000"]
LAMB1 = BASE + ["--compress", "sign", "--optimizer", "onebit_lamb"]


def _plan(numels):
    offs, o = [], 0
    for n in numels:
        offs.append(o)
        o += (n + 63) // 64 * 64
    return BucketPlan(numels, offs, 1.0, 0, o)


def _bits(a, b):
    return torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def _place(plan, per_tensor, fill=0.0):
    out = torch.full((plan.length,), float(fill))
    for off, vals in zip(plan.offsets, per_tensor):
        out[off:off + len(vals)] = torch.tensor(vals, dtype=torch.float32)
    return out


def test_hand_computed_two_tensors():
    """beta1 = beta2 = 0.5, eps = 0, one rank: every intermediate up to f_raw is exact in fp32.

    Tensor A (adapts, 2 elements), tensor B (does not, 2 elements).  The payload encodes
    [2, -2 | 4, -4]: each chunk's scale is its mean |e|, so m = [2, -2 | 4, -4].
    g = (m - m_old / 2) / (1 / 2):  m_old = [0, 4 | 0, 0]   ->  g  = [4, -8 | 8, -8]
    vf = vf / 2 + g^2 / 2:          vf   = [16, 64 | 0, 0]  ->  vf = [16, 64 | 32, 32]
    q = sqrt(v) / sqrt(vf):         v    = [4, 256 | 1, 0]  ->  q  = [2 / 4, 16 / 8] = [0.5, 2]
    A: f_raw = 2, last_factor 1 -> f = 1 + 0.1 (the upper band), r = r_frozen * f = 3 * f.
    B: r = 1, last_factor stays 7; its second coordinate has v = 0 and keeps its parameter."""
    plan = _plan([2, 2])
    lay = Layout.build("sign", plan)
    recv = oracle.encode_sign(_place(plan, [[2.0, -2.0], [4.0, -4.0]]), plan, lay)[None]
    gap = 123.0  # positions between the tensors: never touched
    p = _place(plan, [[1.0, 1.0], [1.0, 1.0]], gap)
    m = _place(plan, [[0.0, 4.0], [0.0, 0.0]], gap)
    v = _place(plan, [[4.0, 256.0], [1.0, 0.0]], gap)
    vf = _place(plan, [[16.0, 64.0], [0.0, 0.0]], gap)
    tensors = [(plan.offsets[0], 2, True), (plan.offsets[1], 2, False)]
    r_frozen = torch.tensor([3.0, 5.0])
    last = torch.tensor([1.0, 7.0])
    lr, wd, step, Tw = 0.25, 0.5, 2, 1
    ratios, factors = oracle.onebit_lamb_apply(recv, plan, lay, p, m, v, vf, tensors, r_frozen,
                                               last, 1.0, lr, 0.5, 0.5, 0.0, wd, step, Tw)
    oA, oB = plan.offsets
    assert m[oA:oA + 2].tolist() == [2.0, -2.0] and m[oB:oB + 2].tolist() == [4.0, -4.0]
    assert vf[oA:oA + 2].tolist() == [16.0, 64.0] and vf[oB:oB + 2].tolist() == [32.0, 32.0]
    f = F(1.0) + F(0.1)  # last_factor * (1 + threshold) < min(max(2, 0.5), 4)
    assert factors.tolist() == [float(f), 7.0] and last.tolist() == [1.0, 7.0]
    assert ratios.tolist() == [float(F(3.0) * f), 1.0]
    bc1, bc2 = F(1 - 0.5 ** step), F(1 - 0.5 ** Tw)

    def stepped(mi, vi, r):
        u = (F(mi) / bc1) / F(math.sqrt(F(vi) / bc2)) + F(wd) * F(1.0)
        return float(F(1.0) - (F(lr) * F(r)) * u)

    rA = F(3.0) * f
    assert p[oA:oA + 2].tolist() == [stepped(2.0, 4.0, rA), stepped(-2.0, 256.0, rA)]
    assert p[oB:oB + 2].tolist() == [stepped(4.0, 1.0, 1.0), 1.0]
    inside = torch.zeros(plan.length, dtype=torch.bool)
    inside[oA:oA + 2] = inside[oB:oB + 2] = True
    for t in (p, m, v, vf):
        assert bool((t[~inside] == gap).all())
    assert v[oA:oA + 2].tolist() == [4.0, 256.0]  # the frozen variance is only read


def _random_case(numels, seed=0, N=2):
    plan = _plan(numels)
    lay = Layout.build("sign", plan)
    gen = torch.Generator().manual_seed(seed)
    recv = torch.stack([oracle.encode_sign(torch.randn(plan.length, generator=gen) * (2.0 ** r),
                                           plan, lay) for r in range(N)])
    p = torch.randn(plan.length, generator=gen)
    m = torch.randn(plan.length, generator=gen) * 0.1
    v = torch.rand(plan.length, generator=gen) + 0.5
    vf = torch.rand(plan.length, generator=gen) + 0.5
    return plan, lay, recv, p, m, v, vf


def test_zero_variance_coordinates_and_tensors():
    """v == 0: the parameter stays, exp_avg and exp_avg_sq_fresh move.  A tensor whose v is all
    zero takes r_frozen and keeps its last_factor.  Gaps are untouched."""
    plan, lay, recv, p, m, v, vf = _random_case([300, 70, 9000])
    o0, o1, o2 = plan.offsets
    v[o0:o0 + 300:3] = 0.0
    v[o1:o1 + 70] = 0.0
    tensors = [(o0, 300, True), (o1, 70, True), (o2, 9000, True)]
    r_frozen = torch.tensor([0.7, 0.3, 1.9])
    last = torch.tensor([1.0, 2.5, 1.0])
    p0, m0, v0, vf0 = (t.clone() for t in (p, m, v, vf))
    ratios, factors = oracle.onebit_lamb_apply(recv, plan, lay, p, m, v, vf, tensors, r_frozen,
                                               last, 0.5, 1e-2, 0.9, 0.999, 1e-8, 0.01, 9, 4)
    inside = torch.zeros(plan.length, dtype=torch.bool)
    for off, n, _ in tensors:
        inside[off:off + n] = True
    dead = inside & (v0 == 0)
    assert _bits(p[dead], p0[dead]) and bool((p[inside & (v0 > 0)] != p0[inside & (v0 > 0)]).all())
    assert bool((m[dead] != m0[dead]).all()) and bool((vf[dead] != vf0[dead]).all())
    assert _bits(m[inside], oracle.decode_sum(recv, plan, lay, 0, 0.5)[inside])
    for t, t0 in ((p, p0), (m, m0), (v, v0), (vf, vf0)):
        assert _bits(t[~inside], t0[~inside])
    assert _bits(v, v0)
    assert float(ratios[1]) == float(r_frozen[1]) and float(factors[1]) == 2.5
    assert float(factors[0]) != 1.0 and float(ratios[0]) == float(F(r_frozen[0]) * F(factors[0]))
    # a NaN in the fresh variance does not enter the maximum
    p2, m2, vf2 = p0.clone(), m0.clone(), vf0.clone()
    vf2[o2 + 17] = float("nan")
    r2, f2 = oracle.onebit_lamb_apply(recv, plan, lay, p2, m2, v0.clone(), vf2, tensors, r_frozen,
                                      last, 0.5, 1e-2, 0.9, 0.999, 1e-8, 0.01, 9, 4)
    assert math.isfinite(float(f2[2])) and float(f2[2]) == float(factors[2])
    assert torch.isnan(vf2[o2 + 17]) and torch.isfinite(p2).all()


def test_every_clamp_branch():
    """Five adapting tensors whose variance ratio is planted: v = k^2 with vf ~ 1.06 after the
    step, so q ~ k / 1.03 over the whole tensor.  Each branch is asserted to exist from the raw
    factor, recomputed here from the fresh variance the oracle stored."""
    n = 200
    plan, lay, recv, p, m, v, vf = _random_case([n] * 5, seed=4, N=1)
    m.zero_()
    vf.fill_(1.0)
    ks = [0.3, 6.0, 1.03, 2.0, 0.6]
    last = torch.tensor([0.5, 4.0, 1.0, 1.0, 1.0])
    for off, k in zip(plan.offsets, ks):
        v[off:off + n] = k * k
    tensors = [(off, n, True) for off in plan.offsets]
    r_frozen = torch.full((5,), 2.0)
    eps = 1e-8
    ratios, factors = oracle.onebit_lamb_apply(recv, plan, lay, p, m, v, vf, tensors, r_frozen,
                                               last, 1.0, 1e-3, 0.9, 0.999, eps, 0.0, 3, 2)
    raw = []
    for off in plan.offsets:
        sl = slice(off, off + n)
        q = (v[sl].double().sqrt().float() + F(eps)) / (vf[sl].double().sqrt().float() + F(eps))
        raw.append(F(q.max()))
    lo, hi = F(1.0) - F(0.1), F(1.0) + F(0.1)
    assert raw[0] < 0.5 and float(factors[0]) == 0.5  # below factor_min
    assert raw[1] > 4.0 and float(factors[1]) == 4.0  # above factor_max
    assert F(1.0) * lo < raw[2] < F(1.0) * hi and float(factors[2]) == float(raw[2])
    assert 0.5 < raw[3] < 4.0 and raw[3] > hi and float(factors[3]) == float(hi)  # upper band
    assert 0.5 < raw[4] < 4.0 and raw[4] < lo and float(factors[4]) == float(lo)  # lower band
    for t in range(5):
        assert float(ratios[t]) == float(F(2.0) * F(factors[t]))
    assert last.tolist() == [0.5, 4.0, 1.0, 1.0, 1.0]  # the caller's row is only read


def _flat():
    from ewdml.models import build_model
    from ewdml.parallel.flat import FlatModel

    torch.manual_seed(0)
    return FlatModel(build_model("LeNet"), bucket_bytes=16 << 20)


def test_warmup_is_flat_lamb_and_the_freeze():
    from ewdml.optim import make_optimizer

    Tw = 3
    fa, fb = _flat(), _flat()
    a = make_optimizer("lamb", fa, lr=2e-3, weight_decay=5e-4)
    b = make_optimizer("onebit_lamb", fb, lr=2e-3, weight_decay=5e-4, freeze_step=Tw)
    assert b.onebit and b.onebit_kind == "lamb" and b.coeff_beta == 0.9
    assert (b.factor_min, b.factor_max, b.factor_threshold) == (0.5, 4.0, 0.1)
    gen = torch.Generator().manual_seed(3)
    seen = []
    for _ in range(Tw):
        assert not b.frozen
        g = torch.randn(fa.numel, generator=gen) * 0.01
        a.step(g)
        b.step(g.clone())
        assert _bits(a.ratio, b.ratio)
        seen.append(b.ratio.double().clone())
    assert b.frozen and b.steps == Tw
    for x, y in ((fa.data, fb.data), (a.exp_avg, b.exp_avg), (a.exp_avg_sq, b.exp_avg_sq)):
        assert _bits(x, y)
    # closed forms, in double: every fp32 step of the recurrence rounds once per operation, two
    # operations per step and the final divide
    ema = sum(0.1 * 0.9 ** (Tw - 1 - k) * r for k, r in enumerate(seen))
    tol = (2 * Tw + 2) * 2.0 ** -24
    torch.testing.assert_close(b.coeff_ema.double(), ema, rtol=tol, atol=0)
    torch.testing.assert_close(b.r_frozen.double(), ema / (1 - 0.9 ** Tw), rtol=tol, atol=0)
    assert _bits(b.exp_avg_sq_fresh, b.exp_avg_sq)
    assert b.exp_avg_sq_fresh.data_ptr() != b.exp_avg_sq.data_ptr()
    assert bool((b.last_factor == 1).all())
    with pytest.raises(RuntimeError, match="freeze"):
        b.step(torch.randn(fa.numel, generator=gen))
    with pytest.raises(RuntimeError, match="freeze"):
        b.step_range(0, fb.numel, torch.zeros(fb.numel))


def test_make_optimizer_refusals():
    from ewdml.optim import make_optimizer
    from ewdml.optim.flat import FlatOnebitLamb

    flat = _flat()
    for bad in (None, 0):
        with pytest.raises(ValueError, match="freeze_step"):
            make_optimizer("onebit_lamb", flat, freeze_step=bad)
    with pytest.raises(ValueError, match="factor"):
        FlatOnebitLamb(flat, freeze_step=2, factor_min=2.0)
    opt = FlatOnebitLamb(flat, freeze_step=2, coeff_beta=0.5, factor_max=8.0)
    assert opt.coeff_beta == 0.5 and opt.factor_max == 8.0
    assert opt.hparams()["factor_max"] == 8.0 and opt.hparams()["t"] == 1


def test_state_dict_round_trip():
    from ewdml.optim import make_optimizer

    fa, fb = _flat(), _flat()
    a = make_optimizer("onebit_lamb", fa, lr=2e-3, freeze_step=2)
    gen = torch.Generator().manual_seed(3)
    for _ in range(2):
        a.step(torch.randn(fa.numel, generator=gen) * 0.01)
    a._factors[1, 0] = 1.5  # state a compressed step would leave
    a.exp_avg_sq_fresh.add_(1e-3)
    sd = a.state_dict()
    assert sd["kind"] == "onebit_lamb" and sd["freeze_step"] == 2 and sd["steps"] == 2
    for k in ("exp_avg_sq_fresh", "coeff_ema", "r_frozen", "last_factor", "exp_avg", "exp_avg_sq",
              "ratio"):
        assert torch.is_tensor(sd[k]), k
    b = make_optimizer("onebit_lamb", fb, lr=1e-3, freeze_step=9)
    b.load_state_dict({k: (v.clone() if torch.is_tensor(v) else v) for k, v in sd.items()})
    assert b.freeze_step == 2 and b.steps == 2 and b.frozen and b.lr == 2e-3
    for name in ("exp_avg", "exp_avg_sq", "exp_avg_sq_fresh", "coeff_ema", "r_frozen", "_factors",
                 "ratio"):
        assert _bits(getattr(a, name), getattr(b, name)), name
    assert not _bits(b.exp_avg_sq_fresh, b.exp_avg_sq)


def test_exchange_refuses_a_wrong_codec():
    from ewdml.compress import Codec
    from ewdml.optim import make_optimizer
    from ewdml.parallel.comm import Comm
    from ewdml.parallel.engine import GradientExchange

    flat = _flat()
    opt = make_optimizer("onebit_lamb", flat, freeze_step=2)
    for codec, ef, pre in ((Codec("qsgd"), True, 1.0), (Codec("sign"), False, 1.0),
                           (Codec("sign"), True, 2.0)):
        with pytest.raises(ValueError, match="1-bit LAMB"):
            GradientExchange(flat, Comm(), codec, opt, overlap=False, error_feedback=ef,
                             predivide=pre, ef_mode="plain")
    with pytest.raises(ValueError, match="sign codec"):
        Codec("qsgd").decode_apply_onebit_lamb(0, None, 1.0, None, None, None, None, {})


def test_cli():
    good = LAMB1 + ["--onebit-warmup-steps", "5"]
    ok = ewdml.parse_args(good + ["--adam-eps", "1e-6", "--clip-grad-norm", "1.0"])
    assert ok.optimizer == "onebit_lamb" and ok.onebit_warmup_steps == 5
    assert ok.adam_eps == 1e-6 and ok.error_feedback is True and ok.clip_grad_norm == 1.0
    adam = ewdml.parse_args(BASE + ["--compress", "sign", "--optimizer", "onebit_adam",
                                    "--onebit-warmup-steps", "5"])
    assert adam.onebit_warmup_steps == 5
    for bad, why in ((["--topology", "ps"], "topology ps"),
                     (["--topology", "sharded"], "topology sharded"),
                     (["--topology", "twostage"], "twostage"),
                     (["--sync-every", "4"], "sync-every"),
                     (["--select-best"], "select-best"),
                     (["--no-error-feedback"], "no-error-feedback"),
                     (["--predivide", "2"], "predivide"),
                     (["--lars-eta", "0.01"], "lars-eta")):
        with pytest.raises(ValueError, match="onebit_lamb .*" + why):
            ewdml.parse_args(good + bad)
    with pytest.raises(ValueError, match="onebit_lamb needs --onebit-warmup-steps"):
        ewdml.parse_args(LAMB1)
    with pytest.raises(ValueError, match="onebit_lamb needs --onebit-warmup-steps"):
        ewdml.parse_args(LAMB1 + ["--onebit-warmup-steps", "0"])
    for codec in ("none", "topk_qsgd", "qsgd", "powersgd"):
        with pytest.raises(ValueError, match="onebit_lamb .*compress sign"):
            ewdml.parse_args(BASE + ["--optimizer", "onebit_lamb", "--onebit-warmup-steps", "5",
                                     "--compress", codec])
    for other in ("adam", "lamb", "sgd"):
        with pytest.raises(ValueError, match="onebit-warmup-steps belongs"):
            ewdml.parse_args(BASE + ["--optimizer", other, "--onebit-warmup-steps", "5"])


def test_trainer_stage_switch_and_frozen_variance():
    """A world of one on the CPU, T_w = 2, 5 steps: the warm-up is the dense LAMB run bit for
    bit, the exchange switches once, exp_avg_sq is bitwise unchanged after step 2 and
    exp_avg_sq_fresh moves."""
    from ewdml.runtime import Trainer

    Tw, steps = 2, 5
    tr = Trainer(ewdml.parse_args(LAMB1 + ["--onebit-warmup-steps", str(Tw), "--max-steps",
                                           str(steps), "--weight-decay", "0.0005"]))
    ref = Trainer(ewdml.parse_args(BASE + ["--compress", "none", "--optimizer", "lamb",
                                           "--max-steps", str(steps), "--weight-decay",
                                           "0.0005"]))
    kinds, switches, prev = [], 0, None
    for _ in range(Tw):
        tr.train_step()
        ref.train_step()
        kinds.append(tr.exchange.codec.kind)
    dense_bytes = tr.exchange.last.payload_bytes
    for x, y in ((tr.flat.data, ref.flat.data), (tr.opt.exp_avg, ref.opt.exp_avg),
                 (tr.opt.exp_avg_sq, ref.opt.exp_avg_sq), (tr.opt.ratio, ref.opt.ratio)):
        assert _bits(x, y)
    v_frozen = tr.opt.exp_avg_sq.clone()
    assert _bits(tr.opt.exp_avg_sq_fresh, v_frozen) and tr.opt.frozen
    r_frozen = tr.opt.r_frozen.clone()
    for t in range(Tw, steps):
        fresh, p_before = tr.opt.exp_avg_sq_fresh.clone(), tr.flat.data.clone()
        tr.train_step()
        kinds.append(tr.exchange.codec.kind)
        assert tr.opt.steps == t + 1
        assert _bits(tr.opt.exp_avg_sq, v_frozen) and _bits(tr.opt.r_frozen, r_frozen)
        assert not torch.equal(tr.opt.exp_avg_sq_fresh, fresh)
        assert not torch.equal(tr.flat.data, p_before)
        assert tr.exchange.last.payload_bytes == sum(
            lay.nbytes for lay in tr.exchange.codec.layouts) < dense_bytes // 20
        lo, hi = tr.opt.trust_ratio_range()
        assert 0 < lo <= hi
        adapts = torch.tensor(tr.opt.adapts)
        f = tr.opt.last_factor
        assert bool((f[~adapts] == 1).all()) and bool(((f >= 0.5) & (f <= 4.0)).all())
        assert _bits(tr.opt.ratio[adapts], (r_frozen * f)[adapts])
        assert bool((tr.opt.ratio[~adapts] == 1).all())
    assert kinds == ["none"] * Tw + ["sign"] * (steps - Tw)
    for a, b in zip(kinds, kinds[1:]):
        switches += a != b
    assert switches == 1
    assert float(tr.exchange.resid.abs().max()) > 0
    assert not _bits(tr.flat.data, ref.flat.data)
    tr.close()
    ref.close()
