"""Adafactor on the CPU: the torch oracle (``compress/oracle.py adafactor_apply``) in double
against the paper's formulas written out per tensor, ``FlatAdafactor``'s state and the command
line."""
import math

import pytest
import torch

import ewdml
from ewdml.compress import oracle
from ewdml.optim import FlatAdafactor, make_optimizer
from tests.layerwise_ref import make_flat, make_grad

BASE = ["--network", "LeNet", "--dataset", "MNIST", "--batch-size", "16", "--synthetic-size",
        "256", "--eval-freq", "0", "--quiet", "--device", "cpu", "--log-interval", "1000"]
HP = dict(lr=0.01, beta1=0.9, clip=0.5, weight_decay=0.01)


def _paper(p, st, g, t, lr, beta1, clip, weight_decay):
    """Algorithms 4 and 5 of the paper for one tensor in float64, lr external, scale-parameter
    on.  The oracle rounds its scalars to fp32, so the two agree to about 1e-7."""
    b2 = 1.0 - t ** -0.8
    q = g * g + 1e-30
    if p.dim() == 2:
        st["R"] = b2 * st["R"] + (1 - b2) * q.mean(dim=1)
        st["C"] = b2 * st["C"] + (1 - b2) * q.mean(dim=0)
        v = torch.outer(st["R"], st["C"]) / st["R"].mean()
    else:
        v = st["v"] = b2 * st["v"] + (1 - b2) * q
    u = g / v.sqrt()
    u = u / max(1.0, math.sqrt(float((u * u).mean())) / clip)
    alpha = lr * max(1e-3, math.sqrt(float((p * p).mean())))
    st["m"] = beta1 * st["m"] + (1 - beta1) * alpha * u
    return p * (1.0 - alpha * weight_decay) - st["m"]


def test_oracle_in_double_follows_the_papers_formulas():
    flat = make_flat(shapes=[(12, 20), (37,)], seed=5)
    ps = [p.detach().double() for p in flat.params]
    sts = [dict(R=torch.zeros(12).double(), C=torch.zeros(20).double(), m=torch.zeros_like(ps[0])),
           dict(v=torch.zeros(37).double(), m=torch.zeros_like(ps[1]))]
    opt = FlatAdafactor(flat, scale_parameter=True, **HP)
    tensors = opt._tensors(0, flat.numel)
    p64, st64 = flat.data.double(), [s.double() for s in (opt.row, opt.col, opt.v, opt.m)]
    for t in (1, 2):
        g = make_grad(flat, t).double() * 0.5
        oracle.adafactor_apply(p64, *st64, g, tensors, step=t, scale_parameter=True, **HP)
        for i, (off, numel, *_) in enumerate(tensors):
            ps[i] = _paper(ps[i], sts[i], g[off:off + numel].view(ps[i].shape), t, **HP)
            torch.testing.assert_close(p64[off:off + numel], ps[i].view(-1), rtol=1e-6, atol=1e-8)
    # the fp32 path steps the same way to fp32 accuracy
    for t in (1, 2):
        opt.step(grad=make_grad(flat, t), grad_scale=0.5)
    torch.testing.assert_close(flat.data.double(), p64, rtol=1e-4, atol=1e-6)


def test_state_is_factored_and_resumes_bitwise():
    flats = [make_flat(bucket_bytes=4 * 8192) for _ in range(3)]
    full, first, rest = (make_optimizer("adafactor", f, lr=0.01, adafactor_beta1=0.9,
                                        weight_decay=0.01) for f in flats)
    assert isinstance(full, FlatAdafactor) and not full.fusable and len(flats[0].buckets) >= 2
    with pytest.raises(ValueError, match="a bucket or the whole model"):
        full.step_range(0, 64, flats[0].grad[:64])
    for s in range(4):
        full.step(grad=make_grad(flats[0], s))
    for s in range(2):  # per bucket, as the exchanges step
        g = make_grad(flats[1], s)
        for b in flats[1].buckets:
            first.step_range(b.start, b.length, g[b.start:b.start + b.length])
        first.end_step()
    sd = {k: (v.clone() if torch.is_tensor(v) else v) for k, v in first.state_dict().items()}
    assert sd["kind"] == "adafactor" and sd["steps"] == 2
    flats[2].data.copy_(flats[1].data)
    rest.load_state_dict(sd)
    for s in range(2, 4):
        rest.step(grad=make_grad(flats[2], s))
    assert torch.equal(flats[2].data.view(torch.int32), flats[0].data.view(torch.int32))
    assert torch.equal(rest.row, full.row) and torch.equal(rest.m, full.m)

    lean = FlatAdafactor(flats[0], lr=0.01)
    sizes = sum(4 * t.numel() for t in (lean.row, lean.col, lean.v))
    assert lean.m is None and lean.state_bytes() == sizes
    # layerwise_ref.SHAPES: the vectors' 10 elements, and n + m floats a matrix, each padded to 4
    assert lean.v.numel() == 12 and lean.row.numel() == 4 + 64 + 4 + 8
    # no element-sized buffer (the (1, 8193) tensor's C is the largest piece of state)
    assert all(t.numel() < flats[0].numel / 2 for t in vars(lean).values() if torch.is_tensor(t))


@pytest.mark.parametrize("flags,match", [
    (["--adafactor-clip", "0.5"], "belongs to --optimizer adafactor"),
    (["--optimizer", "adam", "--adafactor-scale-parameter"], "belongs to --optimizer adafactor"),
    (["--optimizer", "adafactor", "--adafactor-clip", "0"], "--adafactor-clip must be > 0"),
    (["--optimizer", "adafactor", "--adafactor-beta1", "1.0"], "--adafactor-beta1 must lie in"),
    (["--optimizer", "adafactor", "--adafactor-beta1", "-0.1"], "--adafactor-beta1 must lie in")])
def test_cli_refusals(flags, match):
    with pytest.raises(ValueError, match=match):
        ewdml.parse_args(BASE + flags)


def test_cli_resolves():
    c = ewdml.parse_args(BASE + ["--optimizer", "adafactor", "--adafactor-scale-parameter"])
    assert (c.adafactor_beta1, c.adafactor_clip, c.adafactor_scale_parameter) == (0.0, 1.0, True)


def test_plan_names_an_empty_tensor():
    from ewdml import ops
    from ewdml.compress.plan import BucketPlan

    with pytest.raises(ValueError, match="tensor 1 has no elements"):
        ops.AdafactorPlan(BucketPlan([8, 0], [0, 8], 1.0, 0, 8), [0, 0])
