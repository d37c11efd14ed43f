"""The threshold-search sparsifier end to end on the GPU (``--compress thresh``): LeNet under
``--hip-graph full`` whose parameters and residual after six steps are bitwise those of the same
steps with every encode and decode run by the torch oracle (``EWDML_ORACLE=1``), in one captured
graph, with SGD and with Adam (the codec feeds it through ``grad_out``); and LeNet on the golden
MNIST images against the project's 96.5 % held-out floor with the settings of the sign codec's
test (tests/e2e/test_sign_train_gpu.py)."""
import pytest
import torch

import ewdml
from ewdml import ops
from ewdml.compress import codecs
from tests.golden_data import mnist_root

pytestmark = pytest.mark.gpu

SYN = ["--network", "LeNet", "--dataset", "MNIST", "--batch-size", "32", "--synthetic-size",
       "256", "--lr", "0.0625", "--momentum", "0.9", "--eval-freq", "0", "--quiet", "--device",
       "cuda", "--amp", "none", "--graph-warmup", "2", "--compress", "thresh"]
STEPS = 6


def _run(flags, steps, oracle_path, monkeypatch):
    """The trainer's flat parameters after ``steps`` steps.  ``oracle_path``: what EWDML_ORACLE=1
    EWDML_GRAD_VIEWS=1 select (both are read when the process starts, so the test sets what they
    set): the oracle on the device tensors, eager steps."""
    from ewdml.runtime import Trainer

    monkeypatch.setattr(codecs, "_FORCE_ORACLE", oracle_path)
    if oracle_path:
        monkeypatch.setenv("EWDML_GRAD_VIEWS", "1")
    else:
        monkeypatch.delenv("EWDML_GRAD_VIEWS", raising=False)
    torch.manual_seed(0)
    tr = Trainer(ewdml.parse_args(flags + ["--max-steps", str(steps), "--hip-graph",
                                           "off" if oracle_path else "full"]))
    for _ in range(steps):
        loss, _ = tr.train_step()
        assert torch.isfinite(loss.detach()).item()
    torch.cuda.synchronize()
    out = dict(params=tr.flat.data.clone(), resid=tr.exchange.resid.clone(),
               describe=tr.exchange.codec.describe(), mode=tr.graph_mode,
               captured=tr._graphs is not None, captures=tr.captures, ef=tr.exchange.ef_mode)
    tr.close()
    return out


@pytest.mark.parametrize("extra", [[], ["--optimizer", "adam", "--lr", "0.001"]],
                         ids=["sgd", "adam"])
def test_graph_steps_bitwise_the_oracle_path(extra, monkeypatch):
    ops.require()
    flags = SYN + extra
    got = _run(flags, STEPS, False, monkeypatch)
    ref = _run(flags, STEPS, True, monkeypatch)
    assert got["describe"] == "thresh-k0.01" and got["ef"] == "plain"
    assert got["mode"] == "full" and got["captured"] and got["captures"] == 1
    assert ref["mode"] == "off"
    diff = (got["params"].view(torch.int32) != ref["params"].view(torch.int32)).sum().item()
    rel = float((got["params"] - ref["params"]).norm() / ref["params"].norm())
    print(f"thresh {extra}: {diff} of {ref['params'].numel()} parameters differ, rel {rel:.3e}")
    assert diff == 0
    assert torch.equal(got["resid"].view(torch.int32), ref["resid"].view(torch.int32))
    assert float(got["resid"].abs().max()) > 0


LENET = ["--network", "LeNet", "--dataset", "MNIST", "--data-dir", mnist_root(),
         "--holdout-from-test", "1000", "--batch-size", "64", "--lr", "0.01", "--momentum", "0.9",
         "--eval-freq", "0", "--quiet", "--device", "cuda", "--hip-graph", "full",
         "--graph-warmup", "2", "--test-batch-size", "1000", "--compress", "thresh"]


def test_lenet_real_mnist_thresh():
    from ewdml.runtime import Trainer

    ops.require()
    torch.manual_seed(0)
    steps = 1500
    tr = Trainer(ewdml.parse_args(LENET + ["--max-steps", str(steps)]))
    assert tr.exchange.ef_mode == "plain" and tr.exchange.codec.describe() == "thresh-k0.01"
    losses = []
    for _ in range(steps):
        loss, _ = tr.train_step()
        losses.append(loss)
    torch.cuda.synchronize()
    assert tr.graph_mode == "full" and tr._graphs is not None and tr.captures == 1
    assert all(torch.isfinite(v.detach()).item() for v in losses)
    ev = tr.evaluate()
    assert ev["samples"] == 1000
    print(f"thresh: holdout top-1 {ev['top1']:.2f} %")
    tr.close()
    assert ev["top1"] >= 96.5, f"holdout top-1 {ev['top1']:.1f}% < 96.5%"
