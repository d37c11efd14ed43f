"""PowerSGD end to end on the GPU (``--compress powersgd``): split-graph steps against eager steps
bit for bit, four codec launches and two collectives per bucket and step, a resume at step 3
against the uninterrupted run, and LeNet on the golden MNIST images at rank 4 against the
project's 96.5 % held-out floor (tests/e2e/test_gpu_accuracy.py).

Measured accuracy (and the dense run's): profiles/validation/powersgd.md."""
import pytest
import torch

import ewdml
from ewdml import ops
from tests.golden_data import mnist_root
from tests.powersgd_sim import same_bits

pytestmark = pytest.mark.gpu

SYN = ["--network", "LeNet", "--dataset", "MNIST", "--batch-size", "16", "--synthetic-size",
       "1024", "--eval-freq", "0", "--quiet", "--device", "cuda", "--amp", "none", "--lr", "0.05",
       "--momentum", "0.9", "--graph-warmup", "2", "--compress", "powersgd", "--powersgd-rank",
       "2", "--bucket-mb", "0.1", "--no-legacy-ckpt"]


def _trainer(flags, steps):
    from ewdml.runtime import Trainer

    torch.manual_seed(0)
    return Trainer(ewdml.parse_args(flags + ["--max-steps", str(steps)]))


def _run(flags, steps, upto=None):
    tr = _trainer(flags, steps)
    while tr.step < (steps if upto is None else upto):
        tr.train_step()
    torch.cuda.synchronize()
    return tr


def test_split_graph_steps_equal_eager_steps_bitwise():
    from ewdml.parallel.powersgd import PowerSGDExchange

    ops.require()
    ref = _run(SYN + ["--hip-graph", "off"], 6)
    tr = _run(SYN + ["--hip-graph", "auto"], 6)
    assert isinstance(tr.exchange, PowerSGDExchange) and tr.flat.attach_grads
    assert ref.graph_mode == "off" and tr.graph_mode == "split"
    assert tr._graphs is not None and len(tr._graphs) == 2 and tr.captures == 1
    assert len(tr.flat.buckets) > 1
    assert same_bits(tr.flat.data, ref.flat.data), "parameters"
    assert same_bits(tr.opt.mom, ref.opt.mom), "momentum"
    assert same_bits(tr.exchange.resid, ref.exchange.resid), "residual"
    assert same_bits(tr.exchange.q, ref.exchange.q), "warm-start Q"
    assert float(tr.exchange.resid.abs().max()) > 0
    assert tr.exchange.codec.describe() == "powersgd-r2"


def test_four_launches_and_two_collectives_per_bucket_and_step(monkeypatch):
    C = ops.require()
    tr = _trainer(SYN + ["--hip-graph", "off"], 3)
    tr.train_step()
    launches, colls = [], []
    for op, name in enumerate(("project", "orth", "backproject", "decode_apply")):
        real = getattr(C, "psgd_" + name)
        monkeypatch.setattr(ops._C, "psgd_" + name,
                            lambda a, op=op, real=real: (launches.append(op), real(a))[1])
    ar = tr.comm.all_reduce
    monkeypatch.setattr(tr.comm, "all_reduce", lambda t, *a, **k: (colls.append(t.numel()),
                                                                   ar(t, *a, **k))[1])
    tr.train_step()
    torch.cuda.synchronize()
    nb = len(tr.flat.buckets)
    assert nb > 1 and all(t.mats for t in tr.exchange.lr_plans)
    assert len(launches) == 4 * nb and sorted(launches) == sorted([0, 1, 2, 3] * nb)
    assert len(colls) == 2 * nb == tr.exchange.last.collectives
    assert sum(colls) * 4 == tr.exchange.last.payload_bytes
    assert tr.exchange.last.wire_bytes_recv == 0  # a world of one: 2 (N - 1) / N = 0


def test_resume_at_step_3_matches_the_uninterrupted_run(tmp_path):
    ops.require()
    full = _run(SYN + ["--train-dir", str(tmp_path / "a")], 6)
    ck = ["--train-dir", str(tmp_path / "b")]
    first = _run(SYN + ck, 6, upto=3)
    first.save_checkpoint()
    rest = _trainer(SYN + ck + ["--resume"], 6)
    assert rest.step == 3
    assert same_bits(rest.exchange.q, first.exchange.q)
    assert same_bits(rest.exchange.resid, first.exchange.resid)
    while rest.step < 6:
        rest.train_step()
    torch.cuda.synchronize()
    for name, a, b in (("parameters", rest.flat.data, full.flat.data),
                       ("momentum", rest.opt.mom, full.opt.mom),
                       ("residual", rest.exchange.resid, full.exchange.resid),
                       ("Q", rest.exchange.q, full.exchange.q)):
        assert same_bits(a, b), name


LENET = ["--network", "LeNet", "--dataset", "MNIST", "--data-dir", mnist_root(),
         "--holdout-from-test", "1000", "--batch-size", "64", "--lr", "0.01", "--momentum", "0.9",
         "--eval-freq", "0", "--quiet", "--device", "cuda", "--graph-warmup", "2",
         "--test-batch-size", "1000"]


def test_lenet_real_mnist_powersgd_rank4():
    ops.require()
    steps = 1500
    tr = _trainer(LENET + ["--compress", "powersgd", "--powersgd-rank", "4"], steps)
    losses = []
    for _ in range(steps):
        loss, _ = tr.train_step()
        losses.append(loss)
    torch.cuda.synchronize()
    assert tr.graph_mode == "split" and tr._graphs is not None and len(tr._graphs) == 2
    assert all(torch.isfinite(v.detach()).item() for v in losses)
    assert float(tr.exchange.resid.abs().max()) > 0
    # 10,200 floats against 431,080: the byte model of README
    assert tr.exchange.last.payload_bytes == 4 * 10200
    ev = tr.evaluate()
    assert ev["samples"] == 1000
    print(f"powersgd rank 4: holdout top-1 {ev['top1']:.2f} %")
    assert ev["top1"] >= 96.5, f"holdout top-1 {ev['top1']:.1f}% < 96.5%"
