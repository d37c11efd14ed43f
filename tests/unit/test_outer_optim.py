"""The outer optimizer of local SGD (``--outer-optimizer``): the torch oracle against
``torch.optim.SGD`` in float64, its identity setting, and the command line's refusals.

Bound of the oracle against float64 (taken as exact), elementwise, with u = 2^-24.  One outer step
is five fp32 operations, each rounded once::

    t1 = m * mu      m' = t1 + d      t2 = m' * mu      s = d + t2      (sgd: s = m')
    t3 = lr * s      a' = a + t3

* Momentum.  With ``M_k = sum_j mu^(k-j) |d_j|`` (the same recursion on ``|d|``), two roundings a
  sync give by induction ``|m_k - exact| <= ((1 + u)^(2k) - 1) M_k``, i.e. ``2 k u M_k`` to first
  order.
* ``s`` adds two roundings (one for sgd, where it is ``m'`` itself) and ``t3`` one more: with
  ``S_k = |d_k| + (mu + 1) M_k``, which bounds ``|s|`` for both kinds, ``|t3 - exact| <= (2 k + 3)
  u lr S_k``.
* ``a'`` inherits the error of ``a`` and of ``t3`` and is rounded once: ``u |a_k|`` more.

Summed over K = 5 syncs the anchor is within ``(2 K + 3) u sum_k (lr S_k + |a_k|)``; the test
allows ``(2 K + 4) u`` times that sum, the extra u covering the second-order terms.  Where nothing
cancels this is a few ulp of the result.
"""
import pytest
import torch

from ewdml import parse_args
from ewdml.compress import oracle

U = 2.0 ** -24
N = 4099
SYNCS = 5


def _inputs(seed=0):
    g = torch.Generator().manual_seed(seed)
    anchor = torch.randn(N, generator=g)
    deltas = [torch.randn(N, generator=g) * 0.1 for _ in range(SYNCS)]
    return anchor, deltas


def _f32(x):
    return float(torch.tensor(x, dtype=torch.float32))


@pytest.mark.parametrize("mu", [0.0, 0.5, 0.9])
@pytest.mark.parametrize("kind", ["sgd", "nesterov"])
def test_oracle_is_torch_sgd_on_the_negated_delta(kind, mu):
    lr = 0.7
    anchor0, deltas = _inputs()
    lr32, mu32 = _f32(lr), _f32(mu)  # the constants as the fp32 arithmetic sees them
    p = torch.nn.Parameter(anchor0.double())
    # torch refuses nesterov without momentum; the rule itself then reads s = d + m' * 0 = d,
    # plain SGD, which is the reference for that case
    opt = torch.optim.SGD([p], lr=lr32, momentum=mu32, nesterov=kind == "nesterov" and mu > 0)
    anchor, data, m = anchor0.clone(), torch.zeros(N), torch.zeros(N)
    shadow = torch.zeros(N, dtype=torch.bfloat16)
    m_abs, budget = torch.zeros(N, dtype=torch.float64), torch.zeros(N, dtype=torch.float64)
    for d in deltas:
        p.grad = -d.double()
        opt.step()
        oracle.outer_apply(anchor, data, m, d.clone(), lr, mu, kind == "nesterov", shadow=shadow)
        m_abs = m_abs * mu32 + d.double().abs()
        budget += p.detach().abs() + lr32 * (d.double().abs() + (mu32 + 1.0) * m_abs)
        assert torch.equal(data, anchor) and torch.equal(shadow, anchor.bfloat16())
    err = (anchor.double() - p.detach()).abs()
    bound = (2 * SYNCS + 4) * U * budget
    print(f"{kind} mu={mu}: max err {float(err.max()):.3e}, worst err / bound "
          f"{float((err / bound).max()):.3f}, median err in ulp of the result "
          f"{float((err / (U * p.detach().abs())).median()):.2f}")
    assert bool((err <= bound).all())
    if mu32:  # torch's buffer is that of the gradient -d
        ref_m = -opt.state[p]["momentum_buffer"]
        assert bool(((m.double() - ref_m).abs() <= (2 * SYNCS + 1) * U * m_abs).all())


def test_identity_setting_is_bitwise_anchor_plus_delta():
    anchor0, deltas = _inputs(1)
    anchor, data, m = anchor0.clone(), torch.zeros(N), torch.zeros(N)
    want = anchor0.clone()
    for d in deltas:
        d[::7] = 0.0
        d[3::11] = -0.0
        want = want + d
        oracle.outer_apply(anchor, data, m, d, 1.0, 0.0, False)
        assert torch.equal(anchor.view(torch.int32), want.view(torch.int32))
        assert torch.equal(data.view(torch.int32), want.view(torch.int32))
        assert torch.equal(m, d)


def test_oracle_stats_are_the_rows_sums_of_squares():
    n = 2 * 8192 + 20
    g = torch.Generator().manual_seed(2)
    d, m = torch.randn(n, generator=g), torch.randn(n, generator=g)
    anchor, data = torch.randn(n, generator=g), torch.zeros(n)
    stats = torch.full((3, 2), -1.0)
    oracle.outer_apply(anchor, data, m, d, 0.7, 0.9, True, stats=stats)
    for r in range(3):
        sl = slice(r * 8192, min(n, (r + 1) * 8192))
        for k, v in enumerate((d, m)):
            want = float((v[sl].double() ** 2).sum())
            assert abs(float(stats[r, k]) - want) <= U * want  # fp64 sum, rounded once


LOCAL = ["--sync-every", "4", "--sync-mode", "model"]


@pytest.mark.parametrize("flags, msg", [
    (["--outer-optimizer", "sgd", "--sync-mode", "model"], "needs --sync-every > 1"),
    (["--outer-optimizer", "nesterov", "--outer-momentum", "0.9", "--sync-every", "4",
      "--sync-mode", "grad"], "--sync-mode grad exchanges a gradient"),
    (["--outer-optimizer", "sgd", "--sync-every", "4"], "there is no delta"),
    (LOCAL + ["--outer-lr", "0.7"], "--outer-lr belongs to --outer-optimizer"),
    (LOCAL + ["--outer-momentum", "0.9"], "--outer-momentum belongs to --outer-optimizer"),
    (LOCAL + ["--outer-optimizer", "nesterov"], "needs --outer-momentum > 0"),
    (LOCAL + ["--outer-optimizer", "nesterov", "--outer-momentum", "0"],
     "needs --outer-momentum > 0"),
    (LOCAL + ["--outer-optimizer", "sgd", "--outer-lr", "0"], "needs --outer-lr > 0"),
    (LOCAL + ["--outer-optimizer", "sgd", "--outer-lr", "-1"], "needs --outer-lr > 0"),
    (LOCAL + ["--outer-optimizer", "sgd", "--outer-momentum", "1"],
     "needs --outer-momentum in [0, 1)"),
    (LOCAL + ["--outer-optimizer", "sgd", "--outer-momentum", "-0.1"],
     "needs --outer-momentum in [0, 1)"),
])
def test_refusals(flags, msg):
    with pytest.raises(ValueError) as e:
        parse_args(flags)
    assert msg in str(e.value) and "--outer-" in str(e.value)


def test_method_6_with_the_diloco_flags_resolves():
    c = parse_args(["--method", "6", "--outer-optimizer", "nesterov", "--outer-momentum", "0.9",
                    "--outer-lr", "0.7"])
    assert (c.sync_every, c.sync_mode, c.select_best) == (20, "model", True)
    assert (c.outer_optimizer, c.outer_lr, c.outer_momentum) == ("nesterov", 0.7, 0.9)
    assert c.compress == "topk_qsgd" and c.error_feedback
    assert c.resolved().outer_lr == 0.7  # resolving twice changes nothing


def test_defaults_and_accepted_combinations():
    c = parse_args([])
    assert (c.outer_optimizer, c.outer_lr, c.outer_momentum) == ("none", None, None)
    c = parse_args(LOCAL + ["--outer-optimizer", "sgd"])
    assert (c.outer_lr, c.outer_momentum) == (1.0, 0.0)
    for extra in (["--select-best"], ["--compress", "none"], ["--optimizer", "lamb"],
                  ["--optimizer", "lion"], ["--optimizer", "adam"], ["--optimizer", "lars"],
                  ["--compress", "qsgd"], ["--no-error-feedback"]):
        c = parse_args(LOCAL + ["--outer-optimizer", "sgd", "--outer-momentum", "0.5"] + extra)
        assert c.outer_optimizer == "sgd"
