"""The two-stage vote (``--compress vote --vote-exchange twostage``) on CPU/Gloo, through the
trainer: LeNet on synthetic data at worlds 2, 3 and 4 -- replicas stay bitwise identical, every
rank sends and receives 2 (N - 1) P bytes per bucket and step, the odd world's result is bitwise
the all-gather vote's, and a checkpoint taken at step 2 resumes bit for bit with every rank's own
momentum."""
import pytest
import torch

from ..twostage_sim import same_bits
from .helpers import run_world

pytestmark = pytest.mark.slow

STEPS = 4
BASE = ["--network", "LeNet", "--dataset", "MNIST", "--batch-size", "16", "--synthetic-size",
        "512", "--lr", "0.0001", "--eval-freq", "0", "--quiet", "--device", "cpu",
        "--log-interval", "1000", "--compress", "vote", "--optimizer", "lion", "--no-legacy-ckpt",
        "--bucket-mb", "0.1"]


def _train(rank, world, exchange, ckpt_dir, stop_at, resume):
    """Steps up to ``stop_at`` (checkpoint there), or -- ``resume`` -- from the checkpoint on."""
    import ewdml
    from ewdml.runtime import Trainer

    args = BASE + ["--vote-exchange", exchange, "--max-steps", str(STEPS), "--train-dir", ckpt_dir]
    tr = Trainer(ewdml.parse_args(args + (["--resume"] if resume else [])))
    out = {"start": tr.step, "exp_avg_at_start": tr.opt.exp_avg.clone(), "sent": [], "recv": [],
           "kind": type(tr.exchange).__name__, "buckets": len(tr.flat.buckets)}
    while tr.step < stop_at:
        tr.train_step()
        out["sent"].append(tr.exchange.last.wire_bytes_sent)
        out["recv"].append(tr.exchange.last.wire_bytes_recv)
        out["collectives"] = tr.exchange.last.collectives
    out["P"] = [t.P for t in getattr(tr.exchange, "ts", [])]
    out.update(params=tr.flat.data.clone(), exp_avg=tr.opt.exp_avg.clone(), steps=tr.opt.steps)
    if stop_at < STEPS:
        tr.save_checkpoint()
    tr.close()
    return out


@pytest.mark.parametrize("world", [2, 3, 4])
def test_replicas_identical_and_wire_bytes(tmp_path, world):
    res = run_world(_train, world, tmp_path / "ts",
                    args=("twostage", str(tmp_path / "ts" / "ck"), STEPS, False))
    r0 = res[0]
    assert r0["kind"] == "TwoStageVoteExchange" and r0["buckets"] > 1
    assert len(r0["P"]) == r0["buckets"] and all(p > 0 and p % 1024 == 0 for p in r0["P"])
    wire = sum(2 * (world - 1) * p for p in r0["P"])
    for r, out in enumerate(res):
        assert same_bits(out["params"], r0["params"]), f"rank {r}: replicas differ"
        assert out["sent"] == out["recv"] == [wire] * STEPS
        assert out["collectives"] == 2 * out["buckets"] and out["steps"] == STEPS
    assert not torch.equal(res[0]["exp_avg"], res[1]["exp_avg"])  # every rank's own momentum
    assert not same_bits(r0["params"], torch.zeros_like(r0["params"]))
    if world == 3:  # no ties at an odd world: bitwise the all-gather majority vote
        ag = run_world(_train, world, tmp_path / "ag",
                       args=("allgather", str(tmp_path / "ag" / "ck"), STEPS, False))
        assert ag[0]["kind"] == "GradientExchange"
        for out, ref in zip(res, ag):
            assert same_bits(out["params"], ref["params"]), "parameters"
            assert same_bits(out["exp_avg"], ref["exp_avg"]), "momentum"


def test_resume_reproduces_the_uninterrupted_run(tmp_path):
    world = 2
    full = run_world(_train, world, tmp_path / "a",
                     args=("twostage", str(tmp_path / "a" / "ck"), STEPS, False))
    ck = str(tmp_path / "b" / "ck")
    first = run_world(_train, world, tmp_path / "b1", args=("twostage", ck, 2, False))
    rest = run_world(_train, world, tmp_path / "b2", args=("twostage", ck, STEPS, True))
    for r, f, a in zip(rest, full, first):
        assert r["start"] == 2 and r["steps"] == STEPS
        assert same_bits(r["exp_avg_at_start"], a["exp_avg"])  # this rank's own row
        for name in ("params", "exp_avg"):
            assert same_bits(r[name], f[name]), name
    assert not torch.equal(rest[0]["exp_avg_at_start"], rest[1]["exp_avg_at_start"])
