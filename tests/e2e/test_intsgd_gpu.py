"""IntSGD end to end on the GPU (``--compress intsgd``): LeNet under ``--hip-graph auto`` (split
graphs around the eager int8 all-reduces) whose parameters after a handful of steps are bitwise
those of the same steps with every encode, decode and scale update run by the torch oracle
(``EWDML_ORACLE=1``), without and with error feedback; the scale in the trainer's log records; and
LeNet on the golden MNIST images against the dense run of the same recipe, within the margin
measured on the oracle path (profiles/validation/intsgd.md)."""
import math

import pytest
import torch

import ewdml
from ewdml import ops
from ewdml.compress import codecs
from tests.golden_data import mnist_root

pytestmark = pytest.mark.gpu

# lr = 2^-4: lr * d is exact, so the oracle path does not depend on whether torch contracts the
# multiply-add of its ``add_(x, alpha=)`` (the kernels never do)
SYN = ["--network", "LeNet", "--dataset", "MNIST", "--batch-size", "32", "--synthetic-size",
       "1024", "--lr", "0.0625", "--momentum", "0.9", "--eval-freq", "0", "--quiet", "--device",
       "cuda", "--amp", "none", "--graph-warmup", "2", "--compress", "intsgd"]
STEPS = 5


def _run(flags, steps, oracle_path, monkeypatch):
    """The trainer's flat parameters after ``steps`` steps.  ``oracle_path``: what EWDML_ORACLE=1
    selects (read when the process starts, so the test sets what it sets): the oracle on the
    device tensors, eager steps."""
    from ewdml.runtime import Trainer

    monkeypatch.setattr(codecs, "_FORCE_ORACLE", oracle_path)
    torch.manual_seed(0)
    tr = Trainer(ewdml.parse_args(flags + ["--max-steps", str(steps), "--hip-graph",
                                           "off" if oracle_path else "auto"]))
    for _ in range(steps):
        loss, _ = tr.train_step()
        assert torch.isfinite(loss.detach()).item()
    torch.cuda.synchronize()
    resid = tr.exchange.resid
    out = dict(params=tr.flat.data.clone(), resid=None if resid is None else resid.clone(),
               describe=tr.exchange.codec.describe(), mode=tr.graph_mode,
               captured=tr._graphs is not None, health=tr.exchange.codec_health(),
               state=tr.exchange.state(), last=tr.exchange.last)
    tr.close()
    return out


@pytest.mark.parametrize("extra", [[], ["--error-feedback"]], ids=["plain", "ef"])
def test_split_graph_steps_bitwise_the_oracle_path(extra, monkeypatch):
    ops.require()
    flags = SYN + extra
    got = _run(flags, STEPS, False, monkeypatch)
    ref = _run(flags, STEPS, True, monkeypatch)
    assert got["describe"] == "intsgd8"
    assert got["mode"] == "split" and got["captured"] and ref["mode"] == "off"
    diff = (got["params"].view(torch.int32) != ref["params"].view(torch.int32)).sum().item()
    rel = float((got["params"] - ref["params"]).norm() / ref["params"].norm())
    print(f"intsgd {extra}: {diff} of {ref['params'].numel()} parameters differ, rel {rel:.3e}; "
          f"health {got['health']}")
    assert diff == 0
    assert got["state"] == ref["state"] and got["state"]["steps"] == STEPS
    a = got["health"]["intsgd_alpha"]
    assert math.isfinite(a) and a > 0 and 0.0 <= got["health"]["intsgd_sat_frac"] <= 1.0
    assert got["health"] == ref["health"]
    assert got["last"].collectives == 1 and got["last"].wire_bytes_sent == 0  # a world of one
    if extra:
        assert torch.equal(got["resid"].view(torch.int32), ref["resid"].view(torch.int32))
        assert float(got["resid"].abs().max()) > 0
    else:
        assert got["resid"] is None and ref["resid"] is None


def test_log_records_carry_the_scale(tmp_path, monkeypatch):
    """``fit`` writes ``intsgd_alpha`` and ``intsgd_sat_frac`` into every log record: after the
    dense first step, the eager steps and the captured ones."""
    from ewdml.runtime import Trainer

    ops.require()
    monkeypatch.setattr(codecs, "_FORCE_ORACLE", False)
    torch.manual_seed(0)
    tr = Trainer(ewdml.parse_args(SYN + ["--max-steps", "6", "--log-interval", "1", "--train-dir",
                                         str(tmp_path)]))
    recs = []
    record = tr.log.record
    monkeypatch.setattr(tr.log, "record", lambda r: (recs.append(dict(r)), record(r))[1])
    out = tr.fit()
    recs = [r for r in recs if "loss" in r]
    assert [r["step"] for r in recs] == [1, 2, 3, 4, 5, 6] and tr.graph_mode == "split"
    for r in recs:
        assert math.isfinite(r["intsgd_alpha"]) and r["intsgd_alpha"] > 0, r
        assert 0.0 <= r["intsgd_sat_frac"] <= 1.0, r
    assert len({r["intsgd_alpha"] for r in recs}) == len(recs)  # the scale follows the updates
    assert out["last"]["intsgd_alpha"] == recs[-1]["intsgd_alpha"]


LENET = ["--network", "LeNet", "--dataset", "MNIST", "--data-dir", mnist_root(),
         "--holdout-from-test", "1000", "--batch-size", "64", "--lr", "0.01", "--momentum", "0.9",
         "--eval-freq", "0", "--quiet", "--device", "cuda", "--hip-graph", "auto",
         "--graph-warmup", "2", "--test-batch-size", "1000"]
ACC_STEPS = 1500
# Allowed gap, in points of held-out top-1, below the dense run of the same recipe: twice the
# largest |dense - intsgd| seen on the CPU oracle path over three seeds and both error-feedback
# settings (0.3 points; per-seed figures in profiles/validation/intsgd.md)
ACC_MARGIN = 0.6


def _accuracy(flags, split):
    from ewdml.runtime import Trainer

    torch.manual_seed(0)
    tr = Trainer(ewdml.parse_args(LENET + flags + ["--max-steps", str(ACC_STEPS)]))
    losses, sat = [], []
    for i in range(ACC_STEPS):
        loss, _ = tr.train_step()
        losses.append(loss)
        if split and i % 50 == 49:  # the saturated fraction of the last encode, 30 samples
            sat.append(tr.exchange.codec_health()["intsgd_sat_frac"])
    torch.cuda.synchronize()
    assert tr.graph_mode == ("split" if split else "full") and tr._graphs is not None
    assert all(torch.isfinite(v.detach()).item() for v in losses)
    ev = tr.evaluate()
    assert ev["samples"] == 1000
    describe = tr.exchange.codec.describe()
    tr.close()
    return ev["top1"], describe, sat


def test_lenet_real_mnist_intsgd_against_dense(monkeypatch):
    ops.require()
    monkeypatch.setattr(codecs, "_FORCE_ORACLE", False)
    dense, _, _ = _accuracy(["--compress", "none"], False)
    print(f"dense: holdout top-1 {dense:.2f} %")
    got = {}
    for name, flags in (("intsgd", ["--compress", "intsgd"]),
                        ("intsgd_ef", ["--compress", "intsgd", "--error-feedback"])):
        top1, describe, sat = _accuracy(flags, True)
        print(f"{name}: holdout top-1 {top1:.2f} % (dense {dense:.2f} %, gap {dense - top1:+.2f}, "
              f"allowed {ACC_MARGIN:.2f}); saturated fraction mean {sum(sat) / len(sat):.2e} "
              f"max {max(sat):.2e}")
        assert describe == "intsgd8"
        got[name] = top1
    for name, top1 in got.items():
        assert dense - top1 <= ACC_MARGIN, \
            f"{name}: holdout top-1 {top1:.2f}% is {dense - top1:.2f} below dense {dense:.2f}%"
