"""Lion end to end on the GPU: LeNet on the golden MNIST images in full HIP-graph steps, dense
(``--compress none``) and with the 1-bit vote exchange (``--compress vote``), against the project's
96.5 % held-out floor (tests/e2e/test_gpu_accuracy.py); captured steps against eager ones; and two
Gloo ranks sharing ``cuda:0``.

The recipe (lr 1e-4, batch 64, 1500 steps) comes from a plain-torch CPU simulation of the same
arithmetic on the same 9000 / 1000 split, which reached 97.4 to 98.3 % at worlds 1, 2 and 3.
Measured on one MI355X (profiles/validation/lion.md): dense Lion 97.70 %, the vote exchange
98.00 % held-out top-1."""
import pytest
import torch

import ewdml
from ewdml import ops
from tests.distributed.helpers import run_world
from tests.golden_data import mnist_root

pytestmark = pytest.mark.gpu

FLOOR = 96.5  # the report's Method 5 LeNet figure (tests/e2e/test_gpu_accuracy.py)
STEPS = 1500
LENET = ["--network", "LeNet", "--dataset", "MNIST", "--data-dir", mnist_root(),
         "--holdout-from-test", "1000", "--batch-size", "64", "--lr", "0.0001",
         "--optimizer", "lion", "--eval-freq", "0", "--quiet", "--device", "cuda",
         "--hip-graph", "full", "--graph-warmup", "2", "--test-batch-size", "1000"]


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


@pytest.mark.parametrize("compress", ["none", "vote"])
def test_lenet_real_mnist_lion(compress):
    ops.require()
    tr, losses = _run(LENET + ["--compress", compress], STEPS)
    assert tr.graph_mode == "full" and tr._graphs is not None
    assert tr.captures == 1  # one graph from the first captured step on: no warm-up stage
    assert tr.opt.steps == STEPS and int(tr.opt.step_t.item()) == STEPS
    assert tr.exchange.vote is (compress == "vote")
    assert all(v == v and abs(v) != float("inf") for v in losses)
    ev = tr.evaluate()
    assert ev["samples"] == 1000
    print(f"Lion, --compress {compress}: holdout top-1 {ev['top1']:.2f} %")
    tr.close()
    assert ev["top1"] >= FLOOR, f"holdout top-1 {ev['top1']:.1f}% < {FLOOR}%"


SYN = ["--network", "LeNet", "--dataset", "MNIST", "--batch-size", "32", "--synthetic-size",
       "1024", "--lr", "0.0001", "--eval-freq", "0", "--quiet", "--device", "cuda", "--amp",
       "none", "--graph-warmup", "2", "--compress", "vote", "--optimizer", "lion"]


def test_graph_matches_eager():
    ops.require()
    ref, _ = _run(SYN + ["--hip-graph", "off"], 10)
    tr, _ = _run(SYN + ["--hip-graph", "auto"], 10)
    assert tr.graph_mode == "full" and tr._graphs is not None and tr.captures == 1
    assert ref.exchange.vote and tr.exchange.vote
    assert torch.equal(tr.opt.step_t, ref.opt.step_t) and int(tr.opt.step_t.item()) == 10
    rel = float((tr.flat.data - ref.flat.data).norm() / ref.flat.data.norm())
    print(f"graph vs eager: rel {rel:.3e}")
    assert rel < 1e-3, f"params differ from eager by {rel:.2e}"
    ref.close()
    tr.close()


def _train(rank, world, steps):
    import os

    os.environ["LOCAL_RANK"] = "0"  # both ranks share the box's one GPU
    from ewdml.parallel.engine import replica_fingerprint
    from ewdml.runtime import Trainer

    torch.cuda.set_device(0)
    ops.require()
    flags = [f for f in SYN if f not in ("--graph-warmup", "2")]
    tr = Trainer(ewdml.parse_args(flags + ["--graph-warmup", "1", "--batch-size", "16",
                                           "--max-steps", str(steps)]))
    before = tr.flat.data.clone()
    losses = []
    for _ in range(steps):
        loss, _ = tr.train_step()
        losses.append(float(loss.detach()))
    torch.cuda.synchronize()
    return {"fp": replica_fingerprint(tr.flat.data), "m": replica_fingerprint(tr.opt.exp_avg),
            "losses": losses, "moved": not torch.equal(before, tr.flat.data),
            "bytes": tr.exchange.last.payload_bytes, "recv": tr.exchange.last.wire_bytes_recv,
            "chunks": sum(b.plan.num_chunks for b in tr.flat.buckets),
            "vote": tr.exchange.vote}


def test_two_ranks_on_one_gpu_identical(tmp_path):
    res = run_world(_train, 2, tmp_path, args=(6,))

    def key(fp):
        return (repr(fp["sum"]), repr(fp["wsum"]), fp["xor"])

    assert key(res[0]["fp"]) == key(res[1]["fp"])  # replicas
    assert key(res[0]["m"]) != key(res[1]["m"])  # every rank's own momentum
    for r in res:
        assert r["vote"] and r["moved"] and all(l == l for l in r["losses"])
        assert r["bytes"] == res[0]["bytes"] == 1024 * r["chunks"] > 0
        assert r["recv"] == r["bytes"]  # (N - 1) x payload
