"""The IntSGD exchange on CPU/Gloo (``parallel/intsgd.py``): worlds of 2 and 3 run 4 steps of
prescribed gradients over two buckets under momentum 0.9.  The replicas are bit-identical; the
scale is the same on every rank and moves from step to step; parameters, momentum and every rank's
residual equal the numpy simulation of ``tests/intsgd_sim.py`` bit for bit at both worlds (integer
sums have no order); the first step is dense and counted as dense, later steps move L bytes per
bucket; a checkpoint at step 2 resumes bit for bit, without and with error feedback."""
import pytest

from ..intsgd_sim import run_rank, same_bits, simulate
from .helpers import run_world

pytestmark = pytest.mark.slow

STEPS = 4


def _rank(rank, world, ef):
    return run_rank(rank, world, STEPS, ef)


@pytest.mark.parametrize("ef", [False, True], ids=["plain", "ef"])
@pytest.mark.parametrize("world", [2, 3])
def test_replicas_identical_and_equal_to_the_simulation(tmp_path, world, ef):
    res = run_world(_rank, world, tmp_path, args=(ef,))
    sim = simulate(world, STEPS, ef)
    for r, out in enumerate(res):
        assert out["buckets"] == 2
        for name in ("params", "mom"):
            assert same_bits(out[name], res[0][name]), (name, r)
            assert same_bits(out[name], sim[name]), (name, r)
        assert out["alphas"] == res[0]["alphas"] == sim["alphas"]
        assert len(set(out["alphas"])) == STEPS and all(a > 0 for a in out["alphas"])
        assert out["state"]["r"] == sim["r"] and out["state"]["steps"] == STEPS
        # step 1 is dense: one fp32 all-reduce of the flat gradient
        dense = 4 * out["numel"]
        assert out["stats"][0] == (dense, 2 * (world - 1) * dense // world,
                                   2 * (world - 1) * dense // world, 1)
        # later steps: L bytes per bucket, 2 (N - 1) L // N each way, one collective per bucket
        wire = sum(2 * (world - 1) * n // world for n in out["lengths"])
        for st in out["stats"][1:]:
            assert st == (sum(out["lengths"]), wire, wire, len(out["lengths"]))
        if ef:
            assert same_bits(out["resid"], sim["resid"][r]), r
            assert float(out["resid"].abs().max()) > 0
        else:
            assert out["resid"] is None
        assert 0.0 <= out["health"]["intsgd_sat_frac"] < 1.0
    if ef:
        assert not same_bits(res[0]["resid"], res[1]["resid"])  # per-rank state


BASE = ["--network", "LeNet", "--dataset", "MNIST", "--batch-size", "16", "--synthetic-size",
        "512", "--eval-freq", "0", "--quiet", "--device", "cpu", "--log-interval", "1000",
        "--compress", "intsgd", "--no-legacy-ckpt", "--bucket-mb", "0.1", "--lr", "0.05",
        "--momentum", "0.9"]
CK_STEPS = 4


def _train(rank, world, ckpt_dir, stop_at, resume, ef):
    import ewdml
    from ewdml.parallel.intsgd import IntSGDExchange
    from ewdml.runtime import Trainer

    args = BASE + ["--max-steps", str(CK_STEPS), "--train-dir", ckpt_dir]
    args += ["--error-feedback"] if ef else []
    tr = Trainer(ewdml.parse_args(args + (["--resume"] if resume else [])))
    out = {"start": tr.step, "dense": tr.exchange.dense_step}
    while tr.step < stop_at:
        tr.train_step()
    ex = tr.exchange
    assert isinstance(ex, IntSGDExchange) and len(tr.flat.buckets) >= 2
    out.update(params=tr.flat.data.clone(), mom=tr.opt.mom.clone(), state=ex.state(),
               resid=None if ex.resid is None else ex.resid.clone())
    if stop_at < CK_STEPS:
        tr.save_checkpoint()
    tr.close()
    return out


@pytest.mark.parametrize("ef", [False, True], ids=["plain", "ef"])
def test_checkpoint_at_step_2_resumes_bitwise(tmp_path, ef):
    world = 2
    full = run_world(_train, world, tmp_path / "a", args=(str(tmp_path / "a" / "ck"), CK_STEPS,
                                                          False, ef))
    ck = str(tmp_path / "b" / "ck")
    run_world(_train, world, tmp_path / "b1", args=(ck, 2, False, ef))
    rest = run_world(_train, world, tmp_path / "b2", args=(ck, CK_STEPS, True, ef))
    for r, f in zip(rest, full):
        assert r["start"] == 2 and not r["dense"]  # the state came back: no second dense step
        assert r["state"] == f["state"]
        for name in ("params", "mom") + (("resid",) if ef else ()):
            assert same_bits(r[name], f[name]), name
    if ef:
        assert not same_bits(full[0]["resid"], full[1]["resid"])
