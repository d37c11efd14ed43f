"""Distributed Lion's 1-bit vote on CPU/Gloo: 2, 3 and 4 ranks run the real exchange over
LeNet-sized parameters with prescribed gradients -- replicas stay bitwise identical, every rank
keeps its own momentum, the parameters are those of a single-process simulation of the N workers'
oracles and each rank receives (N - 1) payloads per step; through the trainer, a checkpoint taken
at step 3 resumes bit for bit with both ranks' momenta."""
import pytest
import torch

from ..lion_sim import run_rank, same_bits, simulate
from .helpers import run_world

pytestmark = pytest.mark.slow

STEPS = 6


def _rank(rank, world, aggregate):
    return run_rank(rank, world, aggregate, STEPS)


@pytest.mark.parametrize("world,aggregate", [(2, "majority"), (3, "majority"), (4, "majority"),
                                             (4, "average")])
def test_replicas_equal_the_oracle_simulation(tmp_path, world, aggregate):
    res = run_world(_rank, world, tmp_path, args=(aggregate,))
    sim = simulate(world, aggregate, STEPS)
    r0 = res[0]
    assert r0["buckets"] > 1 and r0["payload"] == 1024 * r0["chunks"]
    fps = set()
    for r, out in enumerate(res):
        assert out["fp_params"] == r0["fp_params"]  # replicas: bitwise identical
        assert same_bits(out["params"], r0["params"])
        assert same_bits(out["params"], sim["params"]), f"rank {r}: parameters"
        assert same_bits(out["exp_avg"], sim["exp_avg"][r]), f"rank {r}: momentum"
        assert out["bytes_recv"] == [(world - 1) * out["payload"]] * STEPS
        fps.add((out["fp_exp_avg"]["xor"], repr(out["fp_exp_avg"]["sum"])))
    assert len(fps) == world  # per-rank state: every momentum differs


BASE = ["--network", "LeNet", "--dataset", "MNIST", "--batch-size", "16", "--synthetic-size",
        "512", "--lr", "0.0001", "--eval-freq", "0", "--quiet", "--device", "cpu",
        "--log-interval", "1000", "--compress", "vote", "--optimizer", "lion", "--no-legacy-ckpt"]


def _train(rank, world, ckpt_dir, stop_at, resume):
    """Steps up to ``stop_at`` (checkpoint there), or -- ``resume`` -- from the checkpoint on."""
    import ewdml
    from ewdml.runtime import Trainer

    args = BASE + ["--max-steps", str(STEPS), "--train-dir", ckpt_dir]
    tr = Trainer(ewdml.parse_args(args + (["--resume"] if resume else [])))
    out = {"start": tr.step, "exp_avg_at_start": tr.opt.exp_avg.clone(), "recv": []}
    while tr.step < stop_at:
        tr.train_step()
        out["recv"].append(tr.exchange.last.wire_bytes_recv)
    out["payload"] = sum(lay.nbytes for lay in tr.exchange.codec.layouts)
    out.update(params=tr.flat.data.clone(), exp_avg=tr.opt.exp_avg.clone(), steps=tr.opt.steps)
    if stop_at < STEPS:
        tr.save_checkpoint()
    tr.close()
    return out


def test_vote_resume_recovers_every_ranks_momentum(tmp_path):
    world = 2
    full = run_world(_train, world, tmp_path / "a", args=(str(tmp_path / "a" / "ck"), STEPS, False))
    ck = str(tmp_path / "b" / "ck")
    first = run_world(_train, world, tmp_path / "b1", args=(ck, 3, False))
    rest = run_world(_train, world, tmp_path / "b2", args=(ck, STEPS, True))
    for r, f, a in zip(rest, full, first):
        assert r["start"] == 3 and r["steps"] == STEPS
        assert same_bits(r["exp_avg_at_start"], a["exp_avg"])  # this rank's own row
        for name in ("params", "exp_avg"):
            assert same_bits(r[name], f[name]), name
        assert r["recv"] == [(world - 1) * r["payload"]] * (STEPS - 3)
    assert same_bits(full[0]["params"], full[1]["params"])
    assert not torch.equal(first[0]["exp_avg"], first[1]["exp_avg"])
    assert not torch.equal(rest[0]["exp_avg_at_start"], rest[1]["exp_avg_at_start"])
