"""1-bit Adam on the CPU: the momentum encode and the frozen-variance step of the torch oracle
(compress/oracle.py), ``FlatOnebitAdam`` (optim/flat.py), the trainer's stage switch in a world of
one, and the command line."""
import numpy as np
import pytest
import torch

import ewdml
from ewdml.compress import Codec, oracle
from ewdml.compress.plan import BucketPlan, Layout

PLANS = [[10], [500, 10], [8192 * 3 + 5, 7, 64, 100003]]

BASE = ["--network", "LeNet", "--dataset", "MNIST", "--batch-size", "16", "--synthetic-size",
        "256", "--eval-freq", "0", "--quiet", "--device", "cpu", "--lr", "0.001",
        "--log-interval", "1000"]
ONEBIT = BASE + ["--compress", "sign", "--optimizer", "onebit_adam"]


def _plan(numels):
    offs, o = [], 0
    for n in numels:
        offs.append(o)
        o += (n + 63) // 64 * 64
    return BucketPlan(numels, offs, 1.0, 0, o)


def _rand(plan, seed, scale=1.0):
    g = torch.zeros(plan.length)
    gen = torch.Generator().manual_seed(seed)
    for off, n in zip(plan.offsets, plan.numels):
        g[off:off + n] = torch.randn(n, generator=gen) * scale
    return g


@pytest.mark.parametrize("numels", PLANS)
def test_beta1_zero_is_the_sign_encode(numels):
    """beta1 = 0, wd = 0: u = 0 * m + 1 * g = g exactly (a +/-0 difference changes neither the
    bit nor e - d), so payload and residual are bitwise those of encode_sign."""
    plan = _plan(numels)
    lay = Layout.build("sign", plan)
    g, m = _rand(plan, 1, 0.3), _rand(plan, 2, 5.0)
    r0 = _rand(plan, 3, 0.1)
    ra, rb = r0.clone(), r0.clone()
    for step in range(2):
        a = oracle.encode_sign_momentum(g + step, plan, lay, ra, m, 0.0)
        b = oracle.encode_sign(g + step, plan, lay, rb)
        assert torch.equal(a, b)
        assert torch.equal(ra.view(torch.int32), rb.view(torch.int32))
    assert not torch.equal(ra, r0)


def test_momentum_encode_formula_and_inputs_untouched():
    plan = _plan([500, 10])
    lay = Layout.build("sign", plan)
    g, m, p = _rand(plan, 1), _rand(plan, 2), _rand(plan, 4)
    keep = [t.clone() for t in (g, m, p)]
    r = _rand(plan, 3, 0.1)
    r2 = r.clone()
    b1, wd = 0.9, 5e-4
    pay = oracle.encode_sign_momentum(g, plan, lay, r, m, b1, wd, p)
    for t, k in zip((g, m, p), keep):
        assert torch.equal(t, k)
    gp = g + p * torch.tensor(wd, dtype=torch.float32)
    u = m * torch.tensor(b1, dtype=torch.float32) + gp * (1 - torch.tensor(b1, dtype=torch.float32))
    assert torch.equal(pay, oracle.encode_sign(u, plan, lay, r2))
    assert torch.equal(r, r2)
    with pytest.raises(ValueError, match="error feedback"):
        oracle.encode_sign_momentum(g, plan, lay, None, m, b1)


def test_apply_oracle_zero_variance_and_gaps():
    plan = _plan([500, 10, 8192 + 3])
    lay = Layout.build("sign", plan)
    N = 3
    recv = torch.stack([oracle.encode_sign(_rand(plan, 10 + r, 3.0 ** r), plan, lay,
                                           torch.zeros(plan.length)) for r in range(N)])
    p, v = _rand(plan, 5), _rand(plan, 6).abs()
    v[::3] = 0.0
    m = torch.full((plan.length,), 7.0)
    p0, v0 = p.clone(), v.clone()
    lr_step, eps = 0.01, 1e-8
    oracle.onebit_adam_apply(recv, plan, lay, p, m, v, 1.0 / N, lr_step, eps)
    want_m = oracle.decode_sum(recv, plan, lay, 0, 1.0 / N)
    inside = torch.zeros(plan.length, dtype=torch.bool)
    for off, n in zip(plan.offsets, plan.numels):
        inside[off:off + n] = True
    assert torch.equal(v, v0)
    assert torch.equal(m[inside], want_m[inside]) and bool((m[~inside] == 7.0).all())
    assert bool((want_m[inside] != 0).all())
    still = inside & (v0 == 0)
    assert torch.equal(p[still], p0[still]) and torch.equal(p[~inside], p0[~inside])
    moved = inside & (v0 > 0)
    root = torch.from_numpy(np.sqrt(v0.numpy()))  # numpy's fp32 sqrt is correctly rounded
    want = p0 - (want_m / (root + eps)) * lr_step
    assert torch.equal(p[moved], want[moved]) and not torch.equal(p[moved], p0[moved])


def test_lr_step():
    import math

    got = oracle.onebit_lr_step(1e-3, 0.9, 0.999, 12, 5)
    b1, b2 = float(np.float32(0.9)), float(np.float32(0.999))  # the betas as the kernel holds them
    assert got == 1e-3 * math.sqrt(1 - b2 ** 5) / (1 - b1 ** 12)
    assert got == pytest.approx(1e-3 * math.sqrt(1 - 0.999 ** 5) / (1 - 0.9 ** 12), rel=1e-4)


def _flat():
    from ewdml.models import build_model
    from ewdml.parallel.flat import FlatModel

    torch.manual_seed(0)
    return FlatModel(build_model("LeNet"), bucket_bytes=16 << 20)


def test_flat_onebit_adam_warmup_is_flat_adam():
    from ewdml.optim import make_optimizer

    Tw = 4
    fa, fb = _flat(), _flat()
    assert torch.equal(fa.data, fb.data)
    a = make_optimizer("adam", fa, lr=1e-3, weight_decay=5e-4)
    b = make_optimizer("onebit_adam", fb, lr=1e-3, weight_decay=5e-4, freeze_step=Tw)
    gen = torch.Generator().manual_seed(3)
    for t in range(Tw):
        assert not b.frozen
        g = torch.randn(fa.numel, generator=gen)
        a.step(g)
        b.step(g.clone())
    assert b.frozen and b.steps == Tw
    for x, y in ((fa.data, fb.data), (a.exp_avg, b.exp_avg), (a.exp_avg_sq, b.exp_avg_sq)):
        assert torch.equal(x.view(torch.int32), y.view(torch.int32))
    with pytest.raises(RuntimeError, match="freeze"):
        b.step(torch.randn(fa.numel, generator=gen))


def test_make_optimizer_refusals_and_eps():
    from ewdml.optim import make_optimizer
    from ewdml.optim.flat import FlatOnebitAdam

    flat = _flat()
    with pytest.raises(ValueError, match="AMSGrad"):
        FlatOnebitAdam(flat, amsgrad=True, freeze_step=3)
    with pytest.raises(ValueError, match="AMSGrad"):
        make_optimizer("onebit_adam", flat, amsgrad=True, freeze_step=3)
    for bad in (None, 0):
        with pytest.raises(ValueError, match="freeze_step"):
            make_optimizer("onebit_adam", flat, freeze_step=bad)
    assert make_optimizer("onebit_adam", flat, freeze_step=2, eps=1e-4).eps == 1e-4
    assert make_optimizer("adam", flat, eps=1e-5).eps == 1e-5
    assert make_optimizer("adam", flat).eps == 1e-8


def test_state_dict_round_trip():
    from ewdml.optim import make_optimizer

    fa, fb = _flat(), _flat()
    a = make_optimizer("onebit_adam", fa, lr=2e-3, freeze_step=2)
    gen = torch.Generator().manual_seed(3)
    for _ in range(2):
        a.step(torch.randn(fa.numel, generator=gen))
    sd = a.state_dict()
    assert sd["kind"] == "onebit_adam" and sd["freeze_step"] == 2 and sd["steps"] == 2
    b = make_optimizer("onebit_adam", fb, lr=1e-3, freeze_step=9)
    b.load_state_dict({k: (v.clone() if torch.is_tensor(v) else v) for k, v in sd.items()})
    assert b.freeze_step == 2 and b.steps == 2 and b.frozen and b.lr == 2e-3
    assert torch.equal(a.exp_avg, b.exp_avg) and torch.equal(a.exp_avg_sq, b.exp_avg_sq)
    assert b.lr_step() == a.lr_step() == oracle.onebit_lr_step(2e-3, 0.9, 0.999, 3, 2)


def _trainer(extra, steps):
    from ewdml.runtime import Trainer

    return Trainer(ewdml.parse_args(ONEBIT + extra + ["--max-steps", str(steps)]))


def test_trainer_stage_switch_and_frozen_variance():
    """A world of one on the CPU: steps 1..T_w are the dense Adam run bit for bit; from step
    T_w + 1 the sign exchange runs, exp_avg_sq never changes again, and elements whose variance
    is 0 keep their parameter while their exp_avg moves."""
    from ewdml.runtime import Trainer

    Tw, steps = 3, 7
    tr = _trainer(["--onebit-warmup-steps", str(Tw)], steps)
    ref = Trainer(ewdml.parse_args(BASE + ["--compress", "none", "--optimizer", "adam",
                                           "--max-steps", str(steps)]))
    assert torch.equal(tr.flat.data, ref.flat.data)
    assert not tr._unroll_ok(2, pos=False)
    for _ in range(Tw):
        tr.train_step()
        ref.train_step()
    assert tr.exchange.codec.kind == "none"
    dense_bytes = tr.exchange.last.payload_bytes
    assert dense_bytes == 4 * sum(b.length for b in tr.flat.buckets)
    for x, y in ((tr.flat.data, ref.flat.data), (tr.opt.exp_avg, ref.opt.exp_avg),
                 (tr.opt.exp_avg_sq, ref.opt.exp_avg_sq)):
        assert torch.equal(x.view(torch.int32), y.view(torch.int32))
    # a coordinate that has not seen a gradient: variance 0 at the freeze
    dead = torch.zeros(tr.flat.numel, dtype=torch.bool)
    b0 = tr.flat.buckets[0]
    dead[b0.start + b0.plan.offsets[0]:b0.start + b0.plan.offsets[0] + 5] = True
    tr.opt.exp_avg_sq[dead] = 0.0
    v_frozen = tr.opt.exp_avg_sq.clone()
    p_dead = tr.flat.data[dead].clone()
    for t in range(Tw, steps):
        m_before = tr.opt.exp_avg.clone()
        p_before = tr.flat.data.clone()
        tr.train_step()
        assert tr.exchange.codec.kind == "sign" and tr.opt.steps == t + 1
        assert torch.equal(tr.opt.exp_avg_sq.view(torch.int32), v_frozen.view(torch.int32))
        assert torch.equal(tr.flat.data[dead], p_dead)
        assert not torch.equal(tr.opt.exp_avg[dead], m_before[dead])
        assert not torch.equal(tr.flat.data, p_before)
        assert tr.exchange.last.payload_bytes == sum(
            lay.nbytes for lay in tr.exchange.codec.layouts) < dense_bytes // 20
    assert float(tr.exchange.resid.abs().max()) > 0
    tr.close()
    ref.close()


def test_exchange_refuses_a_wrong_codec():
    from ewdml.optim import make_optimizer
    from ewdml.parallel.comm import Comm
    from ewdml.parallel.engine import GradientExchange

    flat = _flat()
    opt = make_optimizer("onebit_adam", flat, freeze_step=2)
    for codec, ef, pre in ((Codec("qsgd"), True, 1.0), (Codec("sign"), False, 1.0),
                           (Codec("sign"), True, 2.0)):
        with pytest.raises(ValueError, match="1-bit Adam"):
            GradientExchange(flat, Comm(), codec, opt, overlap=False, error_feedback=ef,
                             predivide=pre, ef_mode="plain")
    with pytest.raises(ValueError, match="sign codec"):
        Codec("qsgd").encode_momentum(0, None, None, None, None, 0.9)


def test_cli():
    ok = ewdml.parse_args(ONEBIT + ["--onebit-warmup-steps", "5", "--adam-eps", "1e-6"])
    assert ok.optimizer == "onebit_adam" and ok.onebit_warmup_steps == 5
    assert ok.adam_eps == 1e-6 and ok.error_feedback is True
    assert ewdml.parse_args(BASE).adam_eps == 1e-8
    good = ONEBIT + ["--onebit-warmup-steps", "5"]
    for bad in (["--topology", "ps"], ["--topology", "sharded"], ["--sync-every", "4"],
                ["--select-best"], ["--no-error-feedback"], ["--predivide", "2"]):
        with pytest.raises(ValueError):
            ewdml.parse_args(good + bad)
    with pytest.raises(ValueError, match="onebit-warmup-steps"):
        ewdml.parse_args(ONEBIT)
    with pytest.raises(ValueError, match="onebit-warmup-steps"):
        ewdml.parse_args(ONEBIT + ["--onebit-warmup-steps", "0"])
    for codec in ("none", "topk_qsgd", "qsgd"):
        with pytest.raises(ValueError, match="compress sign"):
            ewdml.parse_args(BASE + ["--optimizer", "onebit_adam", "--onebit-warmup-steps", "5",
                                     "--compress", codec])
    with pytest.raises(ValueError, match="onebit_adam"):
        ewdml.parse_args(BASE + ["--optimizer", "adam", "--onebit-warmup-steps", "5"])
    for name, match in ((["--no-error-feedback"], "error-feedback"), (["--predivide", "2"],
                                                                       "predivide")):
        with pytest.raises(ValueError, match=match):
            ewdml.parse_args(good + name)
