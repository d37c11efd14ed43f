"""Muon on the CPU: the torch oracle (compress/oracle.py muon_apply / muon_orthogonalize) through
``FlatMuon`` against a float64 transcription of the rule, the singular values Newton-Schulz
leaves, the zero input, the command line and the checkpoint round trip."""
import pytest
import torch

import ewdml
from ewdml.compress import oracle
from ewdml.optim import FlatMuon, make_optimizer

from tests.layerwise_ref import make_flat, make_grad, split

BASE = ["--network", "LeNet", "--dataset", "MNIST", "--batch-size", "16", "--synthetic-size",
        "256", "--eval-freq", "0", "--quiet", "--device", "cpu", "--log-interval", "1000"]
A, B, C = 3.4445, -4.7750, 2.0315


def ref64(p, mom, g, shape, lr, momentum, wd, nesterov, aux_lr, steps):
    """One Muon step of one tensor in float64, as the rule is written."""
    mom = momentum * mom + g
    u = g + momentum * mom if nesterov else mom
    if len(shape) < 2:
        return p - aux_lr * (u + wd * p), mom
    n, m = shape[0], p.numel() // shape[0]
    x = u.reshape(n, m) / (u.norm() + 1e-7)
    if n > m:
        x = x.t()
    for _ in range(steps):
        a = x @ x.t()
        b = B * a + C * a @ a
        x = A * x + b @ x
    o = (x.t() if n > m else x).reshape(-1)
    return p * (1 - lr * wd) - lr * max(1.0, n / m) ** 0.5 * o, mom


@pytest.mark.parametrize("wd", [0.0, 1e-2])
@pytest.mark.parametrize("nesterov", [False, True])
def test_oracle_matches_float64(nesterov, wd):
    flat = make_flat(shapes=[(10,), (3, 7), (64, 128), (40, 6), (5, 2, 3, 3)])
    kw = dict(lr=0.02, momentum=0.9, weight_decay=wd, nesterov=nesterov)
    opt = FlatMuon(flat, aux_lr=0.005, ns_steps=5, **kw)
    ps, ms = split(flat, flat.data), split(flat, opt.mom)
    for s in range(3):
        g = make_grad(flat, s)
        opt.step(grad=g, grad_scale=0.5)
        for i, (q, gi) in enumerate(zip(flat.params, split(flat, g))):
            ps[i], ms[i] = ref64(ps[i], ms[i], 0.5 * gi, q.shape, 0.02, 0.9, wd, nesterov,
                                 0.005, 5)
    for got, want in zip(split(flat, flat.data) + split(flat, opt.mom), ps + ms):
        torch.testing.assert_close(got, want, rtol=1e-5, atol=1e-6)


@pytest.mark.parametrize("shape", [(10, 500), (20, 25), (80, 1152), (800, 50)])
def test_singular_values(shape):
    u = torch.randn(shape, generator=torch.Generator().manual_seed(sum(shape)))
    sv = torch.linalg.svdvals(oracle.muon_orthogonalize(u, 5, "fp32").double())
    assert 0.65 < float(sv.min()) and float(sv.max()) < 1.2


@pytest.mark.parametrize("ns_dtype", ["fp32", "bf16"])
def test_zero_input_gives_exact_zero(ns_dtype):
    o = oracle.muon_orthogonalize(torch.zeros(12, 40), 5, ns_dtype)
    assert torch.equal(o, torch.zeros(12, 40))


def test_flags_parse_and_belong_to_muon():
    c = ewdml.parse_args(BASE + ["--optimizer", "muon"])
    assert (c.muon_ns_steps, c.muon_ns_dtype, c.muon_aux_lr) == (5, "fp32", None)
    c = ewdml.parse_args(BASE + ["--optimizer", "muon", "--muon-ns-steps", "3", "--muon-ns-dtype",
                                 "bf16", "--muon-aux-lr", "0.001", "--nesterov", "--momentum",
                                 "0.95"])
    assert (c.muon_ns_steps, c.muon_ns_dtype, c.muon_aux_lr) == (3, "bf16", 0.001)
    for flag, v in (("--muon-ns-steps", "3"), ("--muon-ns-dtype", "bf16"),
                    ("--muon-aux-lr", "0.1")):
        with pytest.raises(ValueError, match=f"{flag} belongs to --optimizer muon"):
            ewdml.parse_args(BASE + ["--optimizer", "lamb", flag, v])
    with pytest.raises(ValueError, match="1..10"):
        ewdml.parse_args(BASE + ["--optimizer", "muon", "--muon-ns-steps", "11"])
    opt = make_optimizer("muon", make_flat(), lr=0.1, momentum=0.9, ns_steps=3, ns_dtype="bf16",
                         aux_lr=0.01, eps=1e-8, eta=None)
    assert isinstance(opt, FlatMuon) and not opt.fusable
    assert (opt.ns_steps, opt.ns_dtype, opt.aux_ratio) == (3, "bf16", 0.01 / 0.1)


@pytest.mark.parametrize("extra", [
    ["--compress", "sign"], ["--compress", "powersgd"], ["--compress", "intsgd"],
    ["--compress", "sign", "--topology", "twostage"], ["--topology", "ps"],
    ["--topology", "sharded"], ["--sync-every", "4"], ["--compress", "topk_qsgd"],
    ["--compress", "vote"], ["--onebit-warmup-steps", "3"], ["--lars-eta", "0.01"],
    ["--clip-grad-norm", "1.0"]])
def test_accepted_and_refused_where_lamb_is(extra):
    outcome = []
    for o in ("lamb", "muon"):
        try:
            ewdml.parse_args(BASE + ["--optimizer", o] + extra)
            outcome.append("ok")
        except ValueError as e:
            outcome.append(str(e).replace(repr(o), "OPT"))  # a message may quote the name
    assert outcome[0] == outcome[1]


def test_checkpoint_round_trip_is_bitwise():
    kw = dict(lr=0.02, momentum=0.9, weight_decay=1e-2, nesterov=True, ns_steps=3, aux_lr=0.01)
    a_flat, b_flat = make_flat(), make_flat()
    a, b = FlatMuon(a_flat, **kw), FlatMuon(b_flat)
    a.step(grad=make_grad(a_flat, 0))
    sd = {k: (v.clone() if torch.is_tensor(v) else v) for k, v in a.state_dict().items()}
    b_flat.data.copy_(a_flat.data)
    b.load_state_dict(sd)
    for o, f in ((a, a_flat), (b, b_flat)):
        o.step(grad=make_grad(f, 1))
    assert b.steps == 2 and b.ns_steps == 3 and b.nesterov
    assert torch.equal(a_flat.data.view(torch.int32), b_flat.data.view(torch.int32))
    assert torch.equal(a.mom.view(torch.int32), b.mom.view(torch.int32))
