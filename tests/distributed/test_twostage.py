"""Two-stage sign all-reduce on CPU/Gloo (``parallel/twostage.py``): worlds of 2, 3 (uneven shards)
and 4 -- buckets of 3 and of 2 chunks, so some ranks own an empty shard -- run 4 steps of
prescribed gradients under SGD and under 1-bit Adam across its switch.  Replicas are bit-identical
and, with both residuals and ``exp_avg``, equal the single-process oracle simulation of all ranks;
the byte counters follow the formula; a checkpoint at step 2 resumes bit for bit."""
import pytest
import torch

from ..twostage_sim import run_rank, same_bits, simulate
from .helpers import run_world

pytestmark = pytest.mark.slow

STEPS = 4


def _rank(rank, world, kind):
    return run_rank(rank, world, kind, STEPS)


@pytest.mark.parametrize("kind", ["sgd", "onebit"])
@pytest.mark.parametrize("world", [2, 3, 4])
def test_replicas_equal_the_oracle_simulation(tmp_path, world, kind):
    res = run_world(_rank, world, tmp_path, args=(kind,))
    sim = simulate(world, kind, STEPS)
    names = ("params", "mom") if kind == "sgd" else ("params", "exp_avg", "exp_avg_sq")
    for r, out in enumerate(res):
        for name in names:
            assert same_bits(out[name], res[0][name]), (name, r)  # replicas
            assert same_bits(out[name], sim[name]), (name, r)
        assert same_bits(out["resid"], sim["resid"][r]), r
        assert same_bits(out["sresid"], sim["sresid"][r]), r
        assert float(out["resid"].abs().max()) > 0
        # bytes: the shard payloads, and 2 (N - 1) P on the wire per bucket and direction
        payload, sent, recv, colls = out["stats"]
        assert payload == sum(sum(row) for row in out["shard_bytes"])
        assert sent == recv == sum(2 * (world - 1) * P for P in out["P"])
        assert colls == 2 * len(out["P"])
        assert all(P == max(row) for P, row in zip(out["P"], out["shard_bytes"]))
    # fewer chunks than ranks: somebody owns an empty shard, whose server residual stays 0
    if world >= 3:
        assert any(0 in row for row in res[0]["shard_bytes"])
    assert any(float(out["sresid"].abs().max()) > 0 for out in res)


BASE = ["--network", "LeNet", "--dataset", "MNIST", "--batch-size", "16", "--synthetic-size",
        "512", "--eval-freq", "0", "--quiet", "--device", "cpu", "--log-interval", "1000",
        "--compress", "sign", "--topology", "twostage", "--no-legacy-ckpt", "--bucket-mb", "0.1"]
OPT = {"sgd": ["--lr", "0.05", "--momentum", "0.9"],
       "onebit": ["--lr", "0.001", "--optimizer", "onebit_adam", "--onebit-warmup-steps", "1"]}


def _train(rank, world, kind, ckpt_dir, stop_at, resume):
    import ewdml
    from ewdml.parallel.twostage import TwoStageSignExchange
    from ewdml.runtime import Trainer

    args = BASE + OPT[kind] + ["--max-steps", str(STEPS), "--train-dir", ckpt_dir]
    tr = Trainer(ewdml.parse_args(args + (["--resume"] if resume else [])))
    out = {"start": tr.step}
    while tr.step < stop_at:
        tr.train_step()
    ex = tr.exchange
    assert isinstance(ex, TwoStageSignExchange)
    out.update(params=tr.flat.data.clone(), resid=ex.resid.clone(), sresid=ex.sresid.clone())
    for k in ("mom", "exp_avg"):
        if getattr(tr.opt, k, None) is not None:
            out[k] = getattr(tr.opt, k).clone()
    if stop_at < STEPS:
        tr.save_checkpoint()
    tr.close()
    return out


@pytest.mark.parametrize("kind", ["sgd", "onebit"])
def test_checkpoint_at_step_2_resumes_bitwise(tmp_path, kind):
    world = 2
    full = run_world(_train, world, tmp_path / "a", args=(kind, str(tmp_path / "a" / "ck"),
                                                          STEPS, False))
    ck = str(tmp_path / "b" / "ck")
    first = run_world(_train, world, tmp_path / "b1", args=(kind, ck, 2, False))
    rest = run_world(_train, world, tmp_path / "b2", args=(kind, ck, STEPS, True))
    for r, f, a in zip(rest, full, first):
        assert r["start"] == 2
        assert float(a["resid"].abs().max()) > 0 and float(a["sresid"].abs().max()) > 0
        for name in f:
            if name != "start":
                assert same_bits(r[name], f[name]), name
    assert not same_bits(full[0]["resid"], full[1]["resid"])  # per-rank state
    assert not same_bits(full[0]["sresid"], full[1]["sresid"])
