"""8-bit Adam end to end on the GPU: LeNet on the synthetic set in full HIP-graph steps, next to
fp32 Adam from the same seed.  The margin is fp32 Adam's own spread (largest minus smallest) of
the same figure over seeds 0, 1 and 2, measured on one MI355X: profiles/validation/adam8.md."""
import pytest
import torch

import ewdml
from ewdml import ops

pytestmark = pytest.mark.gpu

STEPS, LAST = 200, 20
MARGIN = 0.003937  # profiles/validation/adam8.md: 0.004077 (seed 1) - 0.000140 (seed 0)
SYN = ["--network", "LeNet", "--dataset", "MNIST", "--batch-size", "32", "--synthetic-size",
       "1024", "--lr", "0.001", "--eval-freq", "0", "--quiet", "--device", "cuda", "--amp",
       "none", "--graph-warmup", "2", "--hip-graph", "full", "--max-steps", str(STEPS)]


def run(optimizer, seed=0):
    """(trainer, mean loss over the last LAST steps)."""
    from ewdml.runtime import Trainer

    torch.manual_seed(seed)
    tr = Trainer(ewdml.parse_args(SYN + ["--optimizer", optimizer, "--seed", str(seed)]))
    losses = [tr.train_step()[0] for _ in range(STEPS)]
    torch.cuda.synchronize()
    assert tr.graph_mode == "full" and tr._graphs is not None
    assert tr.opt.steps == STEPS == int(tr.opt.step_t)
    tail = [float(v.detach()) for v in losses[-LAST:]]
    assert all(v == v and abs(v) != float("inf") for v in tail)
    return tr, sum(tail) / LAST


def test_lenet_adam8bit_next_to_adam():
    ops.require()
    ref, loss32 = run("adam")
    ref.close()
    tr, loss8 = run("adam8bit")
    print(f"mean loss of the last {LAST} of {STEPS} steps: adam {loss32:.6f}, adam8bit {loss8:.6f}")
    state, n = tr.opt.state_bytes(), tr.flat.numel
    tr.close()
    assert loss8 <= loss32 + MARGIN
    assert state <= 0.27 * 8 * n, f"{state} B of state for {n} elements"
