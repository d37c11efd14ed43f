"""APOLLO end to end on the GPU: LeNet on the synthetic set trains in full HIP-graph steps, and
the captured run is bitwise the eager one past four projection epochs (the signs are redrawn at
steps 9, 17, 25 and 33 from the device step counter, inside the replayed graph).  The dense
exchange: it draws no random numbers, so both runs do the same arithmetic."""
import pytest
import torch

import ewdml

pytestmark = pytest.mark.gpu

STEPS = 36
FLAGS = ["--network", "LeNet", "--dataset", "MNIST", "--batch-size", "16", "--synthetic-size",
         "1024", "--eval-freq", "0", "--quiet", "--device", "cuda", "--amp", "none", "--optimizer",
         "apollo", "--apollo-rank", "16", "--apollo-update-gap", "8", "--lr", "3e-3",
         "--compress", "none", "--graph-warmup", "2", "--max-steps", str(STEPS)]


def _run(graph):
    from ewdml.runtime import Trainer

    torch.manual_seed(0)
    tr = Trainer(ewdml.parse_args(FLAGS + ["--hip-graph", graph]))
    losses = [float(tr.train_step()[0].detach()) for _ in range(STEPS)]
    torch.cuda.synchronize()
    assert tr.opt.kind == "apollo" and tr.opt.steps == STEPS == int(tr.opt.step_t)
    return tr, losses


def test_lenet_trains_and_the_captured_step_is_bitwise_the_eager_one():
    eager, _ = _run("off")
    tr, losses = _run("full")
    assert tr.graph_mode == "full" and tr._graphs is not None
    assert all(l == l and abs(l) != float("inf") for l in losses)
    assert sum(losses[-6:]) < sum(losses[:6])
    assert torch.equal(tr.flat.data.view(torch.int32), eager.flat.data.view(torch.int32))
    for k in tr.opt._STATE:
        assert torch.equal(getattr(tr.opt, k), getattr(eager.opt, k)), k
    eager.close()
    tr.close()
