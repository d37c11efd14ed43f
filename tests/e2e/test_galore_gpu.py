"""GaLore end to end on the GPU: LeNet on the synthetic set trains, and a run saved at step 10 and
resumed is bitwise the straight run, the projectors included (refreshes at steps 1, 9 and 17).
Eager steps (``--hip-graph off``), as Adafactor's resume test."""
import pytest
import torch

import ewdml

pytestmark = pytest.mark.gpu

FLAGS = ["--network", "LeNet", "--dataset", "MNIST", "--batch-size", "16", "--synthetic-size",
         "1024", "--eval-freq", "0", "--quiet", "--device", "cuda", "--amp", "none", "--optimizer",
         "galore", "--galore-rank", "16", "--galore-update-gap", "8", "--lr", "1e-3",
         "--hip-graph", "off", "--no-legacy-ckpt", "--max-steps", "20"]


def _trainer(extra):
    from ewdml.runtime import Trainer

    torch.manual_seed(0)
    return Trainer(ewdml.parse_args(FLAGS + extra))


def test_lenet_trains_and_resumes_bitwise(tmp_path):
    full = _trainer(["--train-dir", str(tmp_path / "a")])
    losses = [float(full.train_step()[0].detach()) for _ in range(20)]
    assert all(l == l and abs(l) != float("inf") for l in losses) and losses[-1] < losses[0]
    first = _trainer(["--train-dir", str(tmp_path / "b")])
    for _ in range(10):
        first.train_step()
    first.save_checkpoint()
    rest = _trainer(["--train-dir", str(tmp_path / "b"), "--resume"])
    assert rest.step == 10 and rest.opt.steps == 10
    while rest.step < 20:
        rest.train_step()
    torch.cuda.synchronize()
    assert torch.equal(rest.flat.data.view(torch.int32), full.flat.data.view(torch.int32))
    assert torch.equal(rest.opt.proj, full.opt.proj) and torch.equal(rest.opt.m_lr, full.opt.m_lr)
