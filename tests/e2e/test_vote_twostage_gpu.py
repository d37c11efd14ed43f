"""The two-stage vote end to end on the GPU (``--compress vote --vote-exchange twostage``).

World 1 through the real communicator: 6 LeNet steps in split graphs are bitwise the all-gather
vote's (``--compress vote``) -- parameters, momentum and the bf16 shadow where there is one; and
three Gloo ranks sharing ``cuda:0`` stay identical and, the world being odd, bitwise equal to the
three ranks of the all-gather vote.

LeNet on the golden MNIST images (the all-gather vote's recipe: lr 1e-4, batch 64, 1500 steps)
against the project's 96.5 % held-out floor (tests/e2e/test_gpu_accuracy.py); at a world of one
the run is the all-gather vote's bit for bit, and so is its accuracy
(profiles/validation/vote_twostage.md)."""
import pytest
import torch

import ewdml
from ewdml import ops
from tests.distributed.helpers import run_world
from tests.golden_data import mnist_root
from tests.twostage_sim import same_bits

pytestmark = pytest.mark.gpu

SYN = ["--network", "LeNet", "--dataset", "MNIST", "--batch-size", "32", "--synthetic-size",
       "1024", "--lr", "0.0001", "--eval-freq", "0", "--quiet", "--device", "cuda", "--amp",
       "none", "--graph-warmup", "2", "--compress", "vote", "--optimizer", "lion",
       "--weight-decay", "0.1", "--bucket-mb", "0.1"]


def _run(flags, steps):
    from ewdml.runtime import Trainer

    torch.manual_seed(0)
    tr = Trainer(ewdml.parse_args(flags + ["--max-steps", str(steps)]))
    for _ in range(steps):
        tr.train_step()
    torch.cuda.synchronize()
    return tr


def test_world_of_one_is_bitwise_the_allgather_vote():
    from ewdml.parallel.twostage import TwoStageVoteExchange

    ops.require()
    ref = _run(SYN, 6)
    tr = _run(SYN + ["--vote-exchange", "twostage"], 6)
    assert isinstance(tr.exchange, TwoStageVoteExchange) and tr.exchange.vote
    assert tr.graph_plan is None and tr.graph_mode == "split"
    assert tr._graphs is not None and len(tr._graphs) == 2 and tr.captures == 1
    assert len(tr.flat.buckets) > 1
    assert int(tr.opt.step_t.item()) == int(ref.opt.step_t.item()) == 6
    assert same_bits(tr.flat.data, ref.flat.data), "parameters"
    assert same_bits(tr.opt.exp_avg, ref.opt.exp_avg), "momentum"
    assert (tr.flat.shadow is None) == (ref.flat.shadow is None)
    if tr.flat.shadow is not None:
        assert torch.equal(tr.flat.shadow.view(torch.int16), ref.flat.shadow.view(torch.int16))
    st = tr.exchange.last
    assert st.wire_bytes_recv == 0 and st.collectives == 2 * len(tr.flat.buckets)
    ref.close()
    tr.close()


FLOOR = 96.5  # the report's Method 5 LeNet figure (tests/e2e/test_gpu_accuracy.py)
LENET = ["--network", "LeNet", "--dataset", "MNIST", "--data-dir", mnist_root(),
         "--holdout-from-test", "1000", "--batch-size", "64", "--lr", "0.0001",
         "--optimizer", "lion", "--eval-freq", "0", "--quiet", "--device", "cuda",
         "--graph-warmup", "2", "--test-batch-size", "1000", "--compress", "vote",
         "--vote-exchange", "twostage"]


def test_lenet_real_mnist_two_stage_vote():
    ops.require()
    tr = _run(LENET, 1500)
    assert tr.graph_mode == "split" and tr.captures == 1 and tr.opt.steps == 1500
    ev = tr.evaluate()
    assert ev["samples"] == 1000
    print(f"two-stage vote: holdout top-1 {ev['top1']:.2f} %")
    tr.close()
    assert ev["top1"] >= FLOOR, f"holdout top-1 {ev['top1']:.1f}% < {FLOOR}%"


def _train(rank, world, exchange, steps):
    import os

    os.environ["LOCAL_RANK"] = "0"  # every rank shares the box's one GPU
    from ewdml.runtime import Trainer

    torch.cuda.set_device(0)
    ops.require()
    flags = [f for f in SYN if f not in ("--graph-warmup", "2")]
    tr = Trainer(ewdml.parse_args(flags + ["--graph-warmup", "1", "--batch-size", "16",
                                           "--vote-exchange", exchange, "--max-steps",
                                           str(steps)]))
    before = tr.flat.data.clone()
    for _ in range(steps):
        tr.train_step()
    torch.cuda.synchronize()
    out = {"params": tr.flat.data.cpu(), "exp_avg": tr.opt.exp_avg.cpu(),
           "moved": not torch.equal(before, tr.flat.data), "graph": tr.graph_mode,
           "kind": type(tr.exchange).__name__, "recv": tr.exchange.last.wire_bytes_recv,
           "P": [t.P for t in getattr(tr.exchange, "ts", [])]}
    tr.close()
    return out


def test_three_ranks_on_one_gpu_equal_the_allgather_vote(tmp_path):
    res = run_world(_train, 3, tmp_path / "ts", args=("twostage", 4))
    ref = run_world(_train, 3, tmp_path / "ag", args=("allgather", 4))
    for r, (out, want) in enumerate(zip(res, ref)):
        assert out["kind"] == "TwoStageVoteExchange" and out["graph"] == "split" and out["moved"]
        assert want["kind"] == "GradientExchange"
        assert same_bits(out["params"], res[0]["params"]), f"rank {r}: replicas differ"
        assert same_bits(out["params"], want["params"]), f"rank {r}: parameters"
        assert same_bits(out["exp_avg"], want["exp_avg"]), f"rank {r}: momentum"
        assert out["recv"] == sum(2 * 2 * p for p in out["P"]) > 0
    assert not torch.equal(res[0]["exp_avg"], res[1]["exp_avg"])  # every rank's own momentum
