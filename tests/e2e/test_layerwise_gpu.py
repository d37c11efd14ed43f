"""LARS and LAMB end to end on the GPU: LeNet on the golden MNIST images in one full HIP-graph
step, LAMB over the sign codec and LARS with momentum over the default codec, held to the
project's 96.5 % held-out floor (tests/e2e/test_gpu_accuracy.py).  Learning rates and the step
count were chosen on the CPU oracle path: profiles/validation/layerwise.md."""
import pytest
import torch

import ewdml
from ewdml import ops
from tests.golden_data import mnist_root

pytestmark = pytest.mark.gpu

STEPS = 1000
LENET = ["--network", "LeNet", "--dataset", "MNIST", "--data-dir", mnist_root(),
         "--holdout-from-test", "1000", "--batch-size", "64", "--eval-freq", "0", "--quiet",
         "--device", "cuda", "--hip-graph", "full", "--graph-warmup", "2", "--test-batch-size",
         "1000", "--max-steps", str(STEPS)]
CASES = {"lamb": ["--optimizer", "lamb", "--compress", "sign", "--lr", "0.003"],
         "lars": ["--optimizer", "lars", "--momentum", "0.9", "--lr", "0.03", "--lars-eta", "0.05"]}


@pytest.mark.parametrize("opt", ["lamb", "lars"])
def test_lenet_real_mnist_layerwise(opt):
    from ewdml.runtime import Trainer

    ops.require()
    torch.manual_seed(0)
    tr = Trainer(ewdml.parse_args(LENET + CASES[opt]))
    assert tr.opt.kind == opt and not tr.opt.fusable
    losses = []
    for _ in range(STEPS):
        loss, _ = tr.train_step()
        losses.append(loss)
    torch.cuda.synchronize()
    assert tr.graph_mode == "full" and tr._graphs is not None
    assert all(torch.isfinite(v.detach()).item() for v in losses)
    assert tr.opt.steps == STEPS == int(tr.opt.step_t)
    lo, hi = tr.opt.trust_ratio_range()
    assert 0 < lo <= hi and lo != 1.0
    ev = tr.evaluate()
    tr.close()
    assert ev["samples"] == 1000
    print(f"{opt}: holdout top-1 {ev['top1']:.2f} %, trust ratios [{lo:.4g}, {hi:.4g}]")
    assert ev["top1"] >= 96.5, f"holdout top-1 {ev['top1']:.1f}% < 96.5%"
