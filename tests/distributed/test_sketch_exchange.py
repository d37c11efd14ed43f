"""The count-sketch exchange on CPU/Gloo (``parallel/sketch.py``): worlds of 2 and 3 run 3 steps of
prescribed gradients over two buckets.  At world 2 (a two-term sum has one order) the parameters,
the momentum and both ranks' residuals equal the numpy simulation of ``tests/sketch_sim.py`` bit for
bit; at world 3 the replicas are bit-identical and every tensor selects exactly its k; a run with
Adam (the non-fusable path) keeps the replicas identical; the byte counters follow the formula; a
checkpoint at step 2 resumes bit for bit."""
import pytest

from ..sketch_sim import make_flat, run_rank, same_bits, simulate
from .helpers import run_world

pytestmark = pytest.mark.slow

STEPS = 3


def _rank(rank, world):
    return run_rank(rank, world, STEPS)


def _rank_adam(rank, world):
    return run_rank(rank, world, STEPS, optimizer="adam")


@pytest.mark.parametrize("world", [2, 3])
def test_replicas_identical_and_equal_to_the_simulation(tmp_path, world):
    res = run_world(_rank, world, tmp_path)
    for r, out in enumerate(res):
        assert out["buckets"] == 2
        for name in ("params", "mom"):
            assert same_bits(out[name], res[0][name]), (name, r)
        assert out["counts"] == out["ks"], r  # selected counts equal k per tensor
        assert float(out["resid"].abs().max()) > 0
        # bytes: 4 (R W + K + dense) per bucket, 2 (N - 1) / N of it on the wire each way
        payload, sent, recv, colls = out["stats"]
        assert payload == sum(4 * f for f in out["floats"])
        assert sent == recv == sum(2 * (world - 1) * 4 * f // world for f in out["floats"])
        assert colls == 2 * len(out["floats"])
    assert not same_bits(res[0]["resid"], res[1]["resid"])  # per-rank state
    if world == 2:
        sim = simulate(world, STEPS)
        for name in ("params", "mom"):
            assert same_bits(res[0][name], sim[name]), name
        for r in range(world):
            assert same_bits(res[r]["resid"], sim["resid"][r]), r


def test_adam_keeps_the_replicas_identical(tmp_path):
    res = run_world(_rank_adam, 2, tmp_path)
    start = make_flat().data
    assert same_bits(res[0]["params"], res[1]["params"])
    assert not same_bits(res[0]["params"], start)
    assert not same_bits(res[0]["resid"], res[1]["resid"])


BASE = ["--network", "LeNet", "--dataset", "MNIST", "--batch-size", "16", "--synthetic-size",
        "512", "--eval-freq", "0", "--quiet", "--device", "cpu", "--log-interval", "1000",
        "--compress", "sketch", "--sketch-rows", "3", "--no-legacy-ckpt", "--bucket-mb", "0.1",
        "--lr", "0.05", "--momentum", "0.9"]
CK_STEPS = 4


def _train(rank, world, ckpt_dir, stop_at, resume):
    import ewdml
    from ewdml.parallel.sketch import SketchExchange
    from ewdml.runtime import Trainer

    args = BASE + ["--max-steps", str(CK_STEPS), "--train-dir", ckpt_dir]
    tr = Trainer(ewdml.parse_args(args + (["--resume"] if resume else [])))
    out = {"start": tr.step}
    while tr.step < stop_at:
        tr.train_step()
    ex = tr.exchange
    assert isinstance(ex, SketchExchange) and len(tr.flat.buckets) >= 2
    out.update(params=tr.flat.data.clone(), resid=ex.resid.clone(), mom=tr.opt.mom.clone())
    if stop_at < CK_STEPS:
        tr.save_checkpoint()
    tr.close()
    return out


def test_checkpoint_at_step_2_resumes_bitwise(tmp_path):
    world = 2
    full = run_world(_train, world, tmp_path / "a", args=(str(tmp_path / "a" / "ck"), CK_STEPS,
                                                          False))
    ck = str(tmp_path / "b" / "ck")
    first = run_world(_train, world, tmp_path / "b1", args=(ck, 2, False))
    rest = run_world(_train, world, tmp_path / "b2", args=(ck, CK_STEPS, True))
    for r, f, a in zip(rest, full, first):
        assert r["start"] == 2 and float(a["resid"].abs().max()) > 0
        for name in ("params", "resid", "mom"):
            assert same_bits(r[name], f[name]), name
    assert not same_bits(full[0]["resid"], full[1]["resid"])
