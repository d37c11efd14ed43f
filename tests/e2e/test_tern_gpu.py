"""The TernGrad codec end to end on the GPU (``--compress tern``): LeNet under ``--hip-graph full``
whose parameters after a handful of steps are bitwise those of the same steps with every encode
and decode run by the torch oracle (``EWDML_ORACLE=1``), without and with error feedback and
without clipping; and LeNet on the golden MNIST images against the dense run of the same recipe,
within the margin measured on the oracle path (profiles/validation/tern.md)."""
import pytest
import torch

import ewdml
from ewdml import ops
from ewdml.compress import codecs
from tests.golden_data import mnist_root

pytestmark = pytest.mark.gpu

SYN = ["--network", "LeNet", "--dataset", "MNIST", "--batch-size", "32", "--synthetic-size",
       "1024", "--lr", "0.0625", "--momentum", "0.9", "--eval-freq", "0", "--quiet", "--device",
       "cuda", "--amp", "none", "--graph-warmup", "2", "--compress", "tern"]
STEPS = 5


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
    resid = tr.exchange.resid
    out = dict(params=tr.flat.data.clone(), resid=None if resid is None else resid.clone(),
               describe=tr.exchange.codec.describe(), mode=tr.graph_mode,
               captured=tr._graphs is not None, ef=tr.exchange.ef_mode)
    tr.close()
    return out


@pytest.mark.parametrize("extra,describe,ef", [
    ([], "tern2b(c=2.5)", None),
    (["--error-feedback"], "tern2b(c=2.5)", "plain"),
    (["--tern-clip", "0"], "tern2b", None),
], ids=["plain", "ef", "noclip"])
def test_graph_steps_bitwise_the_oracle_path(extra, describe, ef, monkeypatch):
    ops.require()
    flags = SYN + extra
    got = _run(flags, STEPS, False, monkeypatch)
    ref = _run(flags, STEPS, True, monkeypatch)
    assert got["describe"] == describe and got["ef"] == ef
    assert got["mode"] == "full" and got["captured"] and ref["mode"] == "off"
    diff = (got["params"].view(torch.int32) != ref["params"].view(torch.int32)).sum().item()
    rel = float((got["params"] - ref["params"]).norm() / ref["params"].norm())
    print(f"tern {extra}: {diff} of {ref['params'].numel()} parameters differ, rel {rel:.3e}")
    assert diff == 0
    if ef:
        assert torch.equal(got["resid"].view(torch.int32), ref["resid"].view(torch.int32))
        assert float(got["resid"].abs().max()) > 0
    else:
        assert got["resid"] is None and ref["resid"] is None


LENET = ["--network", "LeNet", "--dataset", "MNIST", "--data-dir", mnist_root(),
         "--holdout-from-test", "1000", "--batch-size", "64", "--lr", "0.01", "--momentum", "0.9",
         "--eval-freq", "0", "--quiet", "--device", "cuda", "--hip-graph", "full",
         "--graph-warmup", "2", "--test-batch-size", "1000"]
ACC_STEPS = 1500
# Allowed gap, in points of held-out top-1, below the dense run of the same recipe: twice the
# largest |dense - tern| seen on the CPU oracle path over three seeds and both error-feedback
# settings (0.6 points; per-seed figures in profiles/validation/tern.md)
ACC_MARGIN = 1.2


def _accuracy(flags):
    from ewdml.runtime import Trainer

    torch.manual_seed(0)
    tr = Trainer(ewdml.parse_args(LENET + flags + ["--max-steps", str(ACC_STEPS)]))
    losses = []
    for _ in range(ACC_STEPS):
        loss, _ = tr.train_step()
        losses.append(loss)
    torch.cuda.synchronize()
    assert tr.graph_mode == "full" and tr._graphs is not None
    assert all(torch.isfinite(v.detach()).item() for v in losses)
    ev = tr.evaluate()
    assert ev["samples"] == 1000
    describe = tr.exchange.codec.describe()
    tr.close()
    return ev["top1"], describe


def test_lenet_real_mnist_tern_against_dense():
    ops.require()
    dense, _ = _accuracy(["--compress", "none"])
    print(f"dense: holdout top-1 {dense:.2f} %")
    got = {}
    for name, flags in (("tern", ["--compress", "tern"]),
                        ("tern_ef", ["--compress", "tern", "--error-feedback"])):
        top1, describe = _accuracy(flags)
        print(f"{name}: holdout top-1 {top1:.2f} % (dense {dense:.2f} %, gap {dense - top1:+.2f}, "
              f"allowed {ACC_MARGIN:.2f})")
        assert describe == "tern2b(c=2.5)"
        got[name] = top1
    for name, top1 in got.items():
        assert dense - top1 <= ACC_MARGIN, \
            f"{name}: holdout top-1 {top1:.2f}% is {dense - top1:.2f} below dense {dense:.2f}%"
