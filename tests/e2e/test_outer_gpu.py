"""``--outer-optimizer`` end to end on one MI355X: LeNet on synthetic data, a world of one, a sync
every 2 steps, 6 steps -- the captured run with ``k_outer_apply`` against the same captured run
with the torch oracle doing the outer step, the graph count against the run without the flag, the
log records -- then the golden MNIST images against the project's 96.5 % held-out floor.

``EWDML_ORACLE=1`` is set here after the codecs were imported (they read it at import), so it
switches the outer step alone: everything else in the two runs is the same kernels.

The MNIST setting was measured on one MI355X next to the same run without an outer optimizer
(profiles/validation/outer.md)."""
import json
import math

import pytest
import torch

import ewdml
import ewdml.compress.codecs as codecs
from ewdml import ops
from tests.golden_data import mnist_root

pytestmark = pytest.mark.gpu

SYN = ["--network", "LeNet", "--dataset", "MNIST", "--batch-size", "32", "--synthetic-size",
       "1024", "--eval-freq", "0", "--quiet", "--device", "cuda", "--amp", "none",
       "--graph-warmup", "2", "--lr", "0.05", "--hip-graph", "auto", "--sync-every", "2",
       "--sync-mode", "model"]
DILOCO = ["--outer-optimizer", "nesterov", "--outer-lr", "0.7", "--outer-momentum", "0.9"]


def _run(flags, steps):
    from ewdml.runtime import Trainer

    torch.manual_seed(0)
    tr = Trainer(ewdml.parse_args(flags + ["--max-steps", str(steps)]))
    for _ in range(steps):
        tr.train_step()
    torch.cuda.synchronize()
    return tr


def _same(a, b):
    return torch.equal(a.view(torch.int32), b.view(torch.int32))


@pytest.mark.parametrize("outer", [DILOCO, ["--outer-optimizer", "sgd", "--outer-lr", "1.0",
                                            "--outer-momentum", "0.5"]], ids=["nesterov", "sgd"])
def test_captured_kernel_run_is_bitwise_the_oracle_run(outer, monkeypatch):
    ops.require()
    assert not codecs._FORCE_ORACLE
    plain = _run(SYN, 6)
    tr = _run(SYN + outer, 6)
    monkeypatch.setenv("EWDML_ORACLE", "1")
    ref = _run(SYN + outer, 6)
    monkeypatch.delenv("EWDML_ORACLE")
    assert tr.exchange._outer_hip and not ref.exchange._outer_hip
    assert tr.graph_mode == ref.graph_mode == plain.graph_mode == "full"
    assert tr._graphs is not None and tr.captures == ref.captures == plain.captures == 2
    assert _same(tr.flat.data, ref.flat.data)
    assert _same(tr.exchange.anchor, ref.exchange.anchor)
    assert _same(tr.exchange.outer_momentum, ref.exchange.outer_momentum)
    assert float(tr.exchange.outer_momentum.abs().max()) > 0
    assert not _same(tr.flat.data, plain.flat.data)
    # the kernel's tree and the oracle's float64 rows agree on the norms
    for a, b in ((tr.exchange.outer_delta_norm, ref.exchange.outer_delta_norm),
                 (tr.exchange.outer_momentum_norm, ref.exchange.outer_momentum_norm)):
        assert a > 0 and abs(a - b) <= (ops.CLIP_SUM_CHAIN + 1) * 2.0 ** -24 * b


def test_identity_setting_is_bitwise_the_run_without_the_flag():
    ops.require()
    plain = _run(SYN, 6)
    tr = _run(SYN + ["--outer-optimizer", "sgd"], 6)
    assert tr.exchange.outer == ("sgd", 1.0, 0.0) and tr.captures == plain.captures == 2
    assert _same(tr.flat.data, plain.flat.data)
    assert _same(tr.exchange.anchor, plain.exchange.anchor)


def test_log_records_carry_finite_norms(tmp_path):
    from ewdml.runtime import Trainer

    ops.require()
    mf = tmp_path / "m.jsonl"
    tr = Trainer(ewdml.parse_args(SYN + DILOCO + ["--log-interval", "1", "--max-steps", "6",
                                                  "--train-dir", str(tmp_path),
                                                  "--no-legacy-ckpt", "--metrics-file", str(mf)]))
    tr.fit()
    assert tr.graph_mode == "full" and tr.captures == 2
    recs = [json.loads(line) for line in (tmp_path / "m.rank0.jsonl").read_text().splitlines()
            if line.strip()]
    recs = {r["step"]: r for r in recs if "step" in r and "eval" not in r}
    assert sorted(recs) == list(range(1, 7))
    assert "outer_delta_norm" not in recs[1]  # no sync yet
    for s in range(2, 7):
        for k in ("outer_delta_norm", "outer_momentum_norm"):
            assert math.isfinite(recs[s][k]) and recs[s][k] > 0, (s, k)
    assert recs[2]["outer_delta_norm"] == recs[3]["outer_delta_norm"]  # the last sync's value
    assert recs[4]["outer_delta_norm"] != recs[2]["outer_delta_norm"]  # a replay: its own


LENET = ["--network", "LeNet", "--dataset", "MNIST", "--data-dir", mnist_root(),
         "--holdout-from-test", "1000", "--batch-size", "64", "--lr", "0.01", "--momentum", "0.9",
         "--eval-freq", "0", "--quiet", "--device", "cuda", "--hip-graph", "full",
         "--graph-warmup", "2", "--test-batch-size", "1000", "--sync-every", "20", "--sync-mode",
         "model"]
# measured 98.2 % (98.8 % without an outer optimizer; DiLoCo's 0.7 / 0.9 at this inner lr
# diverges to 27 %, at lr / 7 it reaches 96.9 %)
OUTER_MNIST = ["--outer-optimizer", "sgd", "--outer-lr", "1.0", "--outer-momentum", "0.5"]


def test_lenet_real_mnist_outer_optimizer():
    ops.require()
    tr = _run(LENET + OUTER_MNIST, 1500)
    assert tr.cfg.compress == "topk_qsgd" and tr.graph_mode == "full" and tr._graphs is not None
    ev = tr.evaluate()
    print(f"{' '.join(OUTER_MNIST)}: holdout top-1 {ev['top1']:.2f} %, outer momentum norm "
          f"{tr.exchange.outer_momentum_norm:.4f}")
    assert ev["samples"] == 1000
    assert ev["top1"] >= 96.5, f"holdout top-1 {ev['top1']:.1f}% < 96.5%"
