"""The two-stage sign all-reduce end to end on the GPU (``--compress sign --topology twostage``).

World 1 through the real communicator: LeNet on the golden MNIST images, SGD and 1-bit Adam,
against the project's 96.5 % held-out floor (tests/e2e/test_gpu_accuracy.py) -- the run quantises
twice, each time with its own residual; split-graph steps against eager steps, bitwise, over 6
steps (1-bit Adam's cross the switch); and two Gloo ranks sharing ``cuda:0`` under prescribed
gradients against the CPU oracle simulation of both ranks.

Measured accuracies: profiles/validation/twostage.md."""
import pytest
import torch

import ewdml
from ewdml import ops
from tests.distributed.helpers import run_world
from tests.golden_data import mnist_root
from tests.twostage_sim import run_rank, same_bits, simulate

pytestmark = pytest.mark.gpu

FLOOR = 96.5
STEPS, TW = 1500, 300
LENET = ["--network", "LeNet", "--dataset", "MNIST", "--data-dir", mnist_root(),
         "--holdout-from-test", "1000", "--batch-size", "64", "--eval-freq", "0", "--quiet",
         "--device", "cuda", "--graph-warmup", "2", "--test-batch-size", "1000", "--compress",
         "sign", "--topology", "twostage"]
OPT = {"sgd": ["--lr", "0.01", "--momentum", "0.9"],
       "onebit": ["--lr", "0.001", "--optimizer", "onebit_adam", "--onebit-warmup-steps", str(TW)]}


def _run(flags, steps):
    from ewdml.runtime import Trainer

    torch.manual_seed(0)
    tr = Trainer(ewdml.parse_args(flags + ["--max-steps", str(steps)]))
    losses = []
    for _ in range(steps):
        loss, _ = tr.train_step()
        losses.append(loss)
    torch.cuda.synchronize()
    return tr, [float(v.detach()) for v in losses]


@pytest.mark.parametrize("kind", ["sgd", "onebit"])
def test_lenet_real_mnist_twostage(kind):
    from ewdml.parallel.twostage import TwoStageSignExchange

    ops.require()
    tr, losses = _run(LENET + OPT[kind], STEPS)
    assert isinstance(tr.exchange, TwoStageSignExchange)
    assert tr.graph_mode == "split" and tr._graphs is not None and len(tr._graphs) == 2
    assert tr.captures == (2 if kind == "onebit" else 1)
    assert all(v == v and abs(v) != float("inf") for v in losses)
    assert float(tr.exchange.resid.abs().max()) > 0 and float(tr.exchange.sresid.abs().max()) > 0
    ev = tr.evaluate()
    assert ev["samples"] == 1000
    print(f"two-stage sign, {kind}: holdout top-1 {ev['top1']:.2f} %")
    assert ev["top1"] >= FLOOR, f"{kind}: holdout top-1 {ev['top1']:.1f}% < {FLOOR}%"


SYN = ["--network", "LeNet", "--dataset", "MNIST", "--batch-size", "32", "--synthetic-size",
       "1024", "--eval-freq", "0", "--quiet", "--device", "cuda", "--amp", "none",
       "--graph-warmup", "2", "--compress", "sign", "--topology", "twostage", "--bucket-mb", "0.1"]
SYN_OPT = {"sgd": ["--lr", "0.05", "--momentum", "0.9"],
           "onebit": ["--lr", "0.001", "--optimizer", "onebit_adam", "--onebit-warmup-steps", "3"]}


@pytest.mark.parametrize("kind", ["sgd", "onebit"])
def test_split_graph_steps_equal_eager_steps_bitwise(kind):
    ops.require()
    flags = SYN + SYN_OPT[kind]
    ref, _ = _run(flags + ["--hip-graph", "off"], 6)
    tr, _ = _run(flags + ["--hip-graph", "auto"], 6)
    assert ref.graph_mode == "off" and tr.graph_mode == "split" and tr._graphs is not None
    assert len(tr.flat.buckets) > 1
    if kind == "onebit":
        assert tr.captures == 2 and tr.opt.frozen and int(tr.opt.step_t.item()) == 6
        assert same_bits(tr.opt.exp_avg, ref.opt.exp_avg)
    assert same_bits(tr.flat.data, ref.flat.data), "parameters"
    assert same_bits(tr.exchange.resid, ref.exchange.resid), "worker residual"
    assert same_bits(tr.exchange.sresid, ref.exchange.sresid), "server residual"
    assert float(tr.exchange.sresid.abs().max()) > 0


def _rank(rank, world, steps):
    import os

    os.environ["LOCAL_RANK"] = "0"  # both ranks share the box's one GPU
    torch.cuda.set_device(0)
    ops.require()
    out = run_rank(rank, world, "sgd", steps, device="cuda")
    torch.cuda.synchronize()
    return out


def test_two_ranks_on_one_gpu_equal_the_oracle_simulation(tmp_path):
    res = run_world(_rank, 2, tmp_path, args=(4,))
    sim = simulate(2, "sgd", 4)
    for r, out in enumerate(res):
        for name in ("params", "mom"):
            assert same_bits(out[name], res[0][name]), (name, r)
            assert same_bits(out[name], sim[name]), (name, r)
        assert same_bits(out["resid"], sim["resid"][r]), r
        assert same_bits(out["sresid"], sim["sresid"][r]), r
    assert not same_bits(res[0]["resid"], res[1]["resid"])


TWO = ["--network", "LeNet", "--dataset", "MNIST", "--batch-size", "16", "--synthetic-size", "512",
       "--lr", "0.001", "--eval-freq", "0", "--quiet", "--device", "cuda", "--log-interval",
       "1000", "--compress", "sign", "--topology", "twostage", "--graph-warmup", "1",
       "--optimizer", "onebit_adam", "--onebit-warmup-steps", "2"]


def _train(rank, world, steps):
    import os

    os.environ["LOCAL_RANK"] = "0"
    from ewdml.parallel.engine import replica_fingerprint
    from ewdml.runtime import Trainer

    torch.cuda.set_device(0)
    ops.require()
    tr = Trainer(ewdml.parse_args(TWO + ["--max-steps", str(steps)]))
    kinds = []
    for _ in range(steps):
        tr.train_step()
        kinds.append(type(tr.exchange).__name__)
    torch.cuda.synchronize()
    return {"fp": replica_fingerprint(tr.flat.data), "m": replica_fingerprint(tr.opt.exp_avg),
            "kinds": kinds, "graph": tr.graph_mode, "bytes": tr.exchange.last.wire_bytes_recv,
            "resid": replica_fingerprint(tr.exchange.resid)}


def test_two_ranks_onebit_through_the_trainer(tmp_path):
    res = run_world(_train, 2, tmp_path, args=(6,))

    def key(fp):
        return (repr(fp["sum"]), repr(fp["wsum"]), fp["xor"])

    assert key(res[0]["fp"]) == key(res[1]["fp"])
    assert key(res[0]["m"]) == key(res[1]["m"])
    assert key(res[0]["resid"]) != key(res[1]["resid"])
    for r in res:
        assert r["kinds"] == ["GradientExchange"] * 2 + ["TwoStageSignExchange"] * 4
        assert r["graph"] == "split" and r["bytes"] == res[0]["bytes"] > 0
