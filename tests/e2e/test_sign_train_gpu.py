"""The sign codec end to end on the GPU: LeNet on the golden MNIST images in one full HIP-graph
step (the project's 96.5 % held-out floor, tests/e2e/test_gpu_accuracy.py), and two Gloo ranks
sharing ``cuda:0`` whose replicas stay bitwise identical."""
import pytest
import torch

import ewdml
from ewdml import ops
from tests.distributed.helpers import run_world
from tests.golden_data import mnist_root

pytestmark = pytest.mark.gpu

LENET = ["--network", "LeNet", "--dataset", "MNIST", "--data-dir", mnist_root(),
         "--holdout-from-test", "1000", "--batch-size", "64", "--lr", "0.01", "--momentum", "0.9",
         "--eval-freq", "0", "--quiet", "--device", "cuda", "--hip-graph", "full",
         "--graph-warmup", "2", "--test-batch-size", "1000"]


def test_lenet_real_mnist_sign():
    from ewdml.runtime import Trainer

    ops.require()
    torch.manual_seed(0)
    steps = 1500
    tr = Trainer(ewdml.parse_args(LENET + ["--compress", "sign", "--max-steps", str(steps)]))
    assert tr.exchange.ef_mode == "plain" and not tr.exchange.local_apply
    losses = []
    for _ in range(steps):
        loss, _ = tr.train_step()
        losses.append(loss)
    torch.cuda.synchronize()
    assert tr.graph_mode == "full" and tr._graphs is not None
    assert all(torch.isfinite(v.detach()).item() for v in losses)
    ev = tr.evaluate()
    assert ev["samples"] == 1000
    print(f"sign codec: holdout top-1 {ev['top1']:.2f} %")
    assert ev["top1"] >= 96.5, f"holdout top-1 {ev['top1']:.1f}% < 96.5%"


TWO = ["--network", "LeNet", "--dataset", "MNIST", "--batch-size", "16", "--synthetic-size", "512",
       "--momentum", "0.9", "--lr", "0.05", "--eval-freq", "0", "--quiet", "--device", "cuda",
       "--log-interval", "1000", "--compress", "sign", "--graph-warmup", "1"]


def _train(rank, world, steps):
    import os

    os.environ["LOCAL_RANK"] = "0"  # both ranks share the box's one GPU
    from ewdml.parallel.engine import replica_fingerprint
    from ewdml.runtime import Trainer

    torch.cuda.set_device(0)
    ops.require()
    tr = Trainer(ewdml.parse_args(TWO + ["--max-steps", str(steps)]))
    before = tr.flat.data.clone()
    losses = []
    for _ in range(steps):
        loss, _ = tr.train_step()
        losses.append(float(loss.detach()))
    torch.cuda.synchronize()
    return {"fp": replica_fingerprint(tr.flat.data), "losses": losses,
            "moved": not torch.equal(before, tr.flat.data),
            "bytes": tr.exchange.last.payload_bytes, "ef": tr.exchange.ef_mode}


def test_two_ranks_on_one_gpu_identical(tmp_path):
    res = run_world(_train, 2, tmp_path, args=(5,))
    key = [(repr(r["fp"]["sum"]), repr(r["fp"]["wsum"]), r["fp"]["xor"]) for r in res]
    assert key[0] == key[1]
    for r in res:
        assert r["moved"] and all(l == l for l in r["losses"])
        assert r["bytes"] == res[0]["bytes"] > 0 and r["ef"] == "plain"
