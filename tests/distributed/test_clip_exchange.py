"""``--clip-grad-norm`` ahead of every gradient exchange on CPU/Gloo, worlds of 2 and 3: each rank
clips its *own* gradient (the logged norms differ from rank to rank), every rank still decodes the
same bytes, so the replicas stay bit-identical; ``--clip-scale-world`` divides the threshold by
sqrt(N)."""
import json
import math
import os

import pytest
import torch

from .helpers import run_world

pytestmark = pytest.mark.slow

STEPS = 3
C = 0.05  # far below LeNet's first gradient norms (cross-entropy at ln 10): active
BASE = ["--network", "LeNet", "--dataset", "MNIST", "--batch-size", "16", "--synthetic-size",
        "512", "--eval-freq", "0", "--quiet", "--device", "cpu", "--log-interval", "1",
        "--no-legacy-ckpt", "--bucket-mb", "0.1", "--lr", "0.05", "--max-steps", str(STEPS)]
CASES = {
    "none": ["--compress", "none"],
    "sign": ["--compress", "sign"],
    "topk_qsgd": ["--compress", "topk_qsgd"],
    "twostage": ["--compress", "sign", "--topology", "twostage"],
    "powersgd": ["--compress", "powersgd"],
    "onebit_adam": ["--compress", "sign", "--optimizer", "onebit_adam", "--onebit-warmup-steps",
                    "1", "--lr", "0.001"],
}


def _train(rank, world, flags, out_dir):
    import ewdml
    from ewdml.runtime import Trainer

    mf = os.path.join(out_dir, "m.jsonl")
    tr = Trainer(ewdml.parse_args(BASE + flags + ["--train-dir", out_dir, "--metrics-file", mf]))
    assert tr.clipper is not None and len(tr.flat.buckets) > 1
    tr.fit()
    with open(os.path.join(out_dir, f"m.rank{rank}.jsonl")) as f:
        recs = [json.loads(line) for line in f if line.strip()]
    recs = [r for r in recs if "grad_norm" in r]
    return {"params": tr.flat.data.clone(), "runs": tr.clipper.runs,
            "threshold": tr.clipper.max_norm, "kind": tr.exchange.codec.kind,
            "norm": [r["grad_norm"] for r in recs], "coef": [r["clip_coef"] for r in recs]}


@pytest.mark.parametrize("case", list(CASES))
@pytest.mark.parametrize("world", [2, 3])
def test_replicas_identical_and_norms_local(tmp_path, world, case):
    res = run_world(_train, world, tmp_path,
                    args=(CASES[case] + ["--clip-grad-norm", str(C)], str(tmp_path)))
    for r, out in enumerate(res):
        assert torch.equal(out["params"].view(torch.int32), res[0]["params"].view(torch.int32)), r
        assert out["runs"] == STEPS  # exactly once per step (1-bit Adam: across both stages)
        assert len(out["norm"]) == STEPS and out["threshold"] == C
        assert all(v == v and v > 0 for v in out["norm"])
        for n, c in zip(out["norm"], out["coef"]):
            want = min(1.0, C / (n + 1e-6))
            assert abs(c - want) <= 1e-6 * want
    assert any(c < 1 for out in res for c in out["coef"])  # active
    assert len({out["norm"][0] for out in res}) == world  # every rank logs its own norm
    if case == "onebit_adam":
        assert res[0]["kind"] == "sign"  # past the stage switch


def test_clip_scale_world_divides_the_threshold(tmp_path):
    world = 2
    flags = CASES["none"] + ["--clip-grad-norm", str(C)]
    a = run_world(_train, world, tmp_path / "a", args=(flags, str(tmp_path / "a")))
    b = run_world(_train, world, tmp_path / "b",
                  args=(flags + ["--clip-scale-world"], str(tmp_path / "b")))
    for ra, rb in zip(a, b):
        assert ra["threshold"] == C and rb["threshold"] == C / math.sqrt(world)
        assert ra["norm"][0] == rb["norm"][0]  # the same first gradient
        assert ra["coef"][0] < 1 and rb["coef"][0] < 1
        ratio = rb["coef"][0] / ra["coef"][0]
        assert abs(ratio - 1 / math.sqrt(world)) <= 1e-6
