"""8-bit Adam on the CPU: the codebooks, the torch oracle (``compress/oracle.py adam8_apply``)
against the float64 reference of ``tests/adam8_ref.py``, ``FlatAdam8bit`` and the command line."""
import pytest
import torch

import ewdml
from ewdml.compress import oracle
from ewdml.optim import FlatAdam8bit, make_optimizer
from tests import adam8_ref as A
from tests import optim_ref as R
from tests.layerwise_ref import make_flat, make_grad

BASE = ["--network", "LeNet", "--dataset", "MNIST", "--batch-size", "16", "--synthetic-size",
        "256", "--eval-freq", "0", "--quiet", "--device", "cpu", "--log-interval", "1000"]


def test_codebooks():
    map_m, mid_m, map_v, mid_v = books = oracle.adam8_codebooks()
    for got, ref in zip(books, A.books()):
        assert got.dtype == torch.float32 and torch.equal(got.double(), ref)
        assert bool((got[1:] > got[:-1]).all())  # distinct, ascending
    assert map_m.numel() == map_v.numel() == 256 and mid_m.numel() == mid_v.numel() == 255
    assert float(map_m[oracle.ADAM8_ZERO]) == 0.0 and float(map_m[-1]) == 1.0
    assert float(map_m[0]) > -1.0 and float(map_v[0]) == 0.0 and float(map_v[-1]) == 1.0


@pytest.mark.parametrize("wd", [0.0, 1e-2])
@pytest.mark.parametrize("name", list(A.RANGES))
def test_oracle_follows_float64_over_20_steps(name, wd):
    """The oracle's parameters stay within 5 % of the largest single-step update of fp32 Adam
    (``optim_ref.adam32``, unquantised) on the same inputs.  Observed: under 0.001 % where no
    code differs, 0.13 % to 2.2 % where an fp32 ``x`` fell on the other side of a midpoint than
    the float64 one (largest: the three tensors together with weight decay, 2.44e-5 of 1.13e-3)."""
    length, blocks, chunks, pad = A.layout(A.RANGES[name])
    p0, grads = A.inputs(name, 20)
    p, st = p0.clone(), oracle.adam8_state(length, chunks)
    p64, st64 = p0.double(), A.fresh(length, chunks)
    pa, ma, va = p0.clone(), torch.zeros(length), torch.zeros(length)
    largest = 0.0
    for t, g in enumerate(grads, 1):
        oracle.adam8_apply(p, *st, g, blocks, A.HP["lr"], 0.9, 0.999, A.HP["eps"], wd, t)
        A.step64(p64, *st64, g, blocks, t, weight_decay=wd, **A.HP)
        before = pa.clone()
        R.adam32(pa, ma, va, None, g, R.lr_step64(A.HP["lr"], 0.9, 0.999, t), beta1=0.9,
                 beta2=0.999, eps=A.HP["eps"], weight_decay=wd)
        largest = max(largest, float((pa - before).abs().max()))
    worst = R.err(p, p64)
    print(f"{name} wd {wd}: |p - p64| max {worst:.3e} = {100 * worst / largest:.3f} % of {largest:.3e}")
    assert worst <= 0.05 * largest
    assert torch.equal(p[pad], p0[pad]) and bool((st[0][pad] == oracle.ADAM8_ZERO).all())


def test_cli_make_optimizer_state_dict_and_ranges():
    c = ewdml.parse_args(BASE + ["--optimizer", "adam8bit", "--adam-eps", "1e-6"])
    assert c.optimizer == "adam8bit" and c.adam_eps == 1e-6
    flat, flat2 = (make_flat(bucket_bytes=4 * 8192) for _ in range(2))
    opt = make_optimizer("adam8bit", flat, lr=2e-3, eps=1e-6, weight_decay=1e-2, momentum=0.9)
    assert isinstance(opt, FlatAdam8bit) and not opt.fusable and opt.eps == 1e-6
    with pytest.raises(ValueError, match="AMSGrad"):
        make_optimizer("adam8bit", flat, amsgrad=True)
    with pytest.raises(ValueError, match="a bucket or the whole model"):
        opt.step_range(0, 64, flat.grad[:64])
    assert opt.state_bytes() <= 0.27 * 8 * flat.numel and len(flat.buckets) >= 2
    for s in range(2):  # per bucket, as the exchanges step
        g = make_grad(flat, s)
        for b in flat.buckets:
            opt.step_range(b.start, b.length, g[b.start:b.start + b.length])
        opt.end_step()
    sd = {k: (v.clone() if torch.is_tensor(v) else v) for k, v in opt.state_dict().items()}
    assert sd["kind"] == "adam8bit" and sd["steps"] == 2
    flat2.data.copy_(flat.data)
    opt2 = make_optimizer("adam8bit", flat2, lr=123.0, eps=1e-6, weight_decay=1e-2)
    opt2.load_state_dict(sd)
    for o in (opt, opt2):  # the whole model addresses the same absmax slots
        o.step(grad=make_grad(flat, 7))
    assert opt2.steps == 3 and opt2.lr == 2e-3
    assert torch.equal(flat2.data.view(torch.int32), flat.data.view(torch.int32))
    assert torch.equal(opt2.code_m, opt.code_m) and torch.equal(opt2.absmax_v, opt.absmax_v)
