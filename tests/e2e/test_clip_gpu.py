"""``--clip-grad-norm`` end to end on one MI355X: LeNet, synthetic data, at most 8 steps a run --
an inactive clip is bitwise the run without the flag, captured steps equal eager ones and follow
the gradients from replay to replay, a dense SGD step moves the parameters by ``lr * C``, and the
clip runs ahead of the sign / 1-bit Adam, two-stage and PowerSGD exchanges -- then the default
codec on the golden MNIST images against the project's 96.5 % held-out floor.

``C_MNIST`` is the median ``grad_norm`` of the first 100 steps of the same run with the clip
inactive, measured on one MI355X (profiles/validation/clip.md)."""
import json

import pytest
import torch

import ewdml
from ewdml import ops
from tests.golden_data import mnist_root

pytestmark = pytest.mark.gpu

SYN = ["--network", "LeNet", "--dataset", "MNIST", "--batch-size", "32", "--synthetic-size",
       "1024", "--eval-freq", "0", "--quiet", "--device", "cuda", "--amp", "none",
       "--graph-warmup", "2", "--lr", "0.05"]
C = 0.05  # far below LeNet's gradient norms on this data (profiles/validation/clip.md): active


def _run(flags, steps):
    from ewdml.runtime import Trainer

    torch.manual_seed(0)
    tr = Trainer(ewdml.parse_args(flags + ["--max-steps", str(steps)]))
    seen = []
    for _ in range(steps):
        loss, _ = tr.train_step()
        seen.append((loss, None if tr.clipper is None else tr.clipper.plan.state.clone()))
    torch.cuda.synchronize()
    losses = [float(l.detach()) for l, _ in seen]
    states = [None if s is None else tuple(s.tolist()) for _, s in seen]
    return tr, losses, states


def _same(a, b):
    return torch.equal(a.view(torch.int32), b.view(torch.int32))


def test_inactive_clip_is_bitwise_the_run_without_the_flag():
    ops.require()
    flags = SYN + ["--hip-graph", "full"]  # the default codec in its full graph
    ref, _, _ = _run(flags, 8)
    tr, _, states = _run(flags + ["--clip-grad-norm", "1e9"], 8)
    assert ref.cfg.compress == tr.cfg.compress == "topk_qsgd"
    assert ref.graph_mode == tr.graph_mode == "full" and tr._graphs is not None
    assert ref.clipper is None and all(s[1] == 1.0 and s[0] > 0 for s in states)
    assert _same(tr.flat.data, ref.flat.data)
    assert _same(tr.exchange.resid, ref.exchange.resid)


@pytest.mark.parametrize("codec", ["none", "sign"])
def test_eager_and_graph_agree_bitwise_and_replays_follow_the_gradients(codec):
    """The dense exchange and the sign codec: neither draws random numbers, so a captured step
    and an eager one run the same arithmetic and any difference would be the clip's."""
    ops.require()
    flags = SYN + ["--compress", codec, "--clip-grad-norm", str(C)]
    ref, _, eager = _run(flags + ["--hip-graph", "off"], 8)
    tr, _, graph = _run(flags + ["--hip-graph", "full"], 8)
    assert ref.graph_mode == "off" and tr.graph_mode == "full" and tr._graphs is not None
    assert tr.captures == 1 and tr.clipper.runs == 3  # two eager steps and the capture
    assert _same(tr.flat.data, ref.flat.data)
    assert graph == eager
    assert all(c < 1 for _, c in graph)
    assert len({n for n, _ in graph[2:]}) == len(graph[2:])  # every replay: its own norm


def test_captured_run_logs_changing_norms(tmp_path):
    from ewdml.runtime import Trainer

    ops.require()
    mf = tmp_path / "m.jsonl"
    tr = Trainer(ewdml.parse_args(SYN + ["--hip-graph", "full", "--clip-grad-norm", str(C),
                                         "--log-interval", "1", "--max-steps", "8",
                                         "--train-dir", str(tmp_path), "--no-legacy-ckpt",
                                         "--metrics-file", str(mf)]))
    tr.fit()
    assert tr.graph_mode == "full" and tr.captures == 1
    recs = [json.loads(line) for line in (tmp_path / "m.rank0.jsonl").read_text().splitlines()
            if line.strip()]
    recs = [r for r in recs if "grad_norm" in r]
    assert [r["step"] for r in recs] == list(range(1, 9))
    assert recs[4]["grad_norm"] != recs[7]["grad_norm"]  # two replays of the one capture
    for r in recs:
        want = min(1.0, C / (r["grad_norm"] + 1e-6))
        assert r["clip_coef"] < 1 and abs(r["clip_coef"] - want) <= 1e-6 * want


def test_world_of_one_dense_sgd_moves_by_lr_times_c():
    from ewdml.runtime import Trainer

    ops.require()
    torch.manual_seed(0)
    tr = Trainer(ewdml.parse_args(SYN + ["--compress", "none", "--momentum", "0", "--hip-graph",
                                         "off", "--clip-grad-norm", str(C), "--max-steps", "2"]))
    p0 = tr.flat.data.clone()
    tr.train_step()
    torch.cuda.synchronize()
    norm, coef = tr.clipper.last()
    moved = float((tr.flat.data.double() - p0.double()).norm())
    print(f"norm {norm:.6f} coef {coef:.6e} |dp| {moved:.9e} lr*C {0.05 * C:.9e}")
    assert coef < 1 and abs(moved - 0.05 * C) <= 1e-5 * 0.05 * C


OTHERS = {
    "onebit_adam": ["--compress", "sign", "--optimizer", "onebit_adam", "--onebit-warmup-steps",
                    "3", "--lr", "0.001"],
    "twostage": ["--compress", "sign", "--topology", "twostage", "--bucket-mb", "0.1"],
    "twostage_onebit": ["--compress", "sign", "--topology", "twostage", "--bucket-mb", "0.1",
                        "--optimizer", "onebit_adam", "--onebit-warmup-steps", "3", "--lr",
                        "0.001"],
    "powersgd": ["--compress", "powersgd", "--bucket-mb", "0.1"],
}


@pytest.mark.parametrize("case", list(OTHERS))
def test_other_exchanges_clip_before_their_encode(case):
    from ewdml.parallel.engine import check_replicas

    ops.require()
    tr, losses, states = _run(SYN + OTHERS[case] + ["--clip-grad-norm", str(C)], 8)
    assert tr.graph_mode in ("full", "split") and tr._graphs is not None
    assert all(v == v and abs(v) != float("inf") for v in losses)
    assert all(c < 1 for _, c in states) and len({n for n, _ in states}) == 8
    if "onebit" in case:  # crossed the stage switch: both stages ran the one clipper
        assert tr.opt.frozen and tr.captures == 2 and tr.exchange.codec.kind == "sign"
        assert tr.exchange.clipper is tr._stages[0].clipper is tr.clipper
    assert float(tr.exchange.resid.abs().max()) > 0
    assert check_replicas(tr.comm, tr.flat.data)["identical"]


C_MNIST = 1.5515551567077637  # median of 100 norms in [1.13, 2.46]
LENET = ["--network", "LeNet", "--dataset", "MNIST", "--data-dir", mnist_root(),
         "--holdout-from-test", "1000", "--batch-size", "64", "--lr", "0.01", "--momentum", "0.9",
         "--eval-freq", "0", "--quiet", "--device", "cuda", "--hip-graph", "full",
         "--graph-warmup", "2", "--test-batch-size", "1000"]


def test_lenet_real_mnist_clipped_default_codec():
    ops.require()
    tr, losses, states = _run(LENET + ["--clip-grad-norm", repr(C_MNIST)], 1000)
    assert tr.cfg.compress == "topk_qsgd" and tr.graph_mode == "full" and tr._graphs is not None
    clipped = sum(c < 1 for _, c in states)
    ev = tr.evaluate()
    print(f"clip {C_MNIST}: {clipped} of 1000 steps clipped, holdout top-1 {ev['top1']:.2f} %")
    assert ev["samples"] == 1000 and clipped >= 1
    assert ev["top1"] >= 96.5, f"holdout top-1 {ev['top1']:.1f}% < 96.5%"
