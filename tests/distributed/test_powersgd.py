"""PowerSGD on CPU/Gloo (``parallel/powersgd.py``): worlds of 2 and 3 run 4 steps of prescribed
gradients over two buckets.  Replicas are bit-identical, ``q`` included; at world 2 (a two-term sum
has one order) the parameters equal the single-process oracle simulation bit for bit; at world 3
the error against the fp64 simulation is within 3 x the fp32 simulation's own + 1e-5; the byte
counters follow the formula; a checkpoint at step 2 resumes bit for bit."""
import pytest
import torch

from ..powersgd_sim import rel, run_rank, same_bits, simulate
from .helpers import run_world

pytestmark = pytest.mark.slow

STEPS = 4


def _rank(rank, world):
    return run_rank(rank, world, STEPS)


@pytest.mark.parametrize("world", [2, 3])
def test_replicas_identical_and_equal_to_the_simulation(tmp_path, world):
    res = run_world(_rank, world, tmp_path)
    sim = simulate(world, STEPS)
    for r, out in enumerate(res):
        assert out["buckets"] == 2
        for name in ("params", "mom"):
            assert same_bits(out[name], res[0][name]), (name, r)
        for a, b in zip(out["q"], res[0]["q"]):
            assert same_bits(a, b), ("q", r)
        assert float(out["resid"].abs().max()) > 0
        # bytes: 4 (p_floats + q_floats) per bucket, 2 (N - 1) / N of it on the wire each way
        payload, sent, recv, colls = out["stats"]
        assert payload == sum(4 * (p + q) for p, q in out["floats"])
        assert sent == recv == sum(2 * (world - 1) * 4 * (p + q) // world
                                   for p, q in out["floats"])
        assert colls == 2 * len(out["floats"])
    assert not same_bits(res[0]["resid"], res[1]["resid"])  # per-rank state
    if world == 2:
        for name in ("params", "mom"):
            assert same_bits(res[0][name], sim[name]), name
        for r in range(world):
            assert same_bits(res[r]["resid"], sim["resid"][r]), r
    else:
        sim64 = simulate(world, STEPS, torch.float64)
        for name in ("params", "mom"):
            ek, eo = rel(res[0][name], sim64[name]), rel(sim[name], sim64[name])
            print(f"{name}: exchange {ek:.3e}, fp32 simulation {eo:.3e}")
            assert ek <= 3 * eo + 1e-5, (name, ek, eo)


BASE = ["--network", "LeNet", "--dataset", "MNIST", "--batch-size", "16", "--synthetic-size",
        "512", "--eval-freq", "0", "--quiet", "--device", "cpu", "--log-interval", "1000",
        "--compress", "powersgd", "--powersgd-rank", "2", "--no-legacy-ckpt", "--bucket-mb", "0.1",
        "--lr", "0.05", "--momentum", "0.9"]


def _train(rank, world, ckpt_dir, stop_at, resume):
    import ewdml
    from ewdml.parallel.powersgd import PowerSGDExchange
    from ewdml.runtime import Trainer

    args = BASE + ["--max-steps", str(STEPS), "--train-dir", ckpt_dir]
    tr = Trainer(ewdml.parse_args(args + (["--resume"] if resume else [])))
    out = {"start": tr.step}
    while tr.step < stop_at:
        tr.train_step()
    ex = tr.exchange
    assert isinstance(ex, PowerSGDExchange) and len(tr.flat.buckets) == 2
    out.update(params=tr.flat.data.clone(), resid=ex.resid.clone(), q=ex.q.clone(),
               mom=tr.opt.mom.clone())
    if stop_at < STEPS:
        tr.save_checkpoint()
    tr.close()
    return out


def test_checkpoint_at_step_2_resumes_bitwise(tmp_path):
    world = 2
    full = run_world(_train, world, tmp_path / "a", args=(str(tmp_path / "a" / "ck"), STEPS,
                                                          False))
    ck = str(tmp_path / "b" / "ck")
    first = run_world(_train, world, tmp_path / "b1", args=(ck, 2, False))
    rest = run_world(_train, world, tmp_path / "b2", args=(ck, STEPS, True))
    for r, f, a in zip(rest, full, first):
        assert r["start"] == 2 and float(a["resid"].abs().max()) > 0
        for name in ("params", "resid", "q", "mom"):
            assert same_bits(r[name], f[name]), name
    assert not same_bits(full[0]["resid"], full[1]["resid"])
    assert same_bits(full[0]["q"], full[1]["q"])
