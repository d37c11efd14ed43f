"""The MXFP8 / MXFP4 codec through the all-gather exchange on CPU/Gloo: 2 and 3 ranks run the real
exchange over LeNet-sized parameters with prescribed gradients -- replicas stay bitwise identical,
every rank keeps its own residual, parameters and momentum are those of a single-process
simulation of the N workers' oracles, and each rank receives (N - 1) payloads of 33/32 (17/32)
bytes per element; and the trainer itself runs LeNet with ``--compress mx``."""
import pytest
import torch

from ..mx_sim import run_rank, same_bits, simulate
from .helpers import run_world

pytestmark = pytest.mark.slow

STEPS = 5


def _rank(rank, world, fmt):
    return run_rank(rank, world, fmt, STEPS)


@pytest.mark.parametrize("fmt", ["fp8", "fp4"])
@pytest.mark.parametrize("world", [2, 3])
def test_replicas_equal_the_oracle_simulation(tmp_path, world, fmt):
    res = run_world(_rank, world, tmp_path, args=(fmt,))
    sim = simulate(world, fmt, STEPS)
    r0 = res[0]
    per = {"fp8": 1.0, "fp4": 0.5}[fmt]
    want = sum((L // 32 + 15) // 16 * 16 + int(L * per) for L in r0["lengths"])
    assert len(r0["lengths"]) > 1 and r0["payload"] == r0["layout_bytes"] == want
    assert r0["describe"] == "mx" + fmt and r0["ef_mode"] == "plain"
    for r, out in enumerate(res):
        assert out["fp_params"] == r0["fp_params"]  # replicas: bitwise identical
        assert same_bits(out["params"], sim["params"]), f"rank {r}: parameters"
        assert same_bits(out["mom"], sim["mom"]), f"rank {r}: momentum"
        assert same_bits(out["resid"], sim["resid"][r]), f"rank {r}: residual"
        assert out["bytes_recv"] == [(world - 1) * out["payload"]] * STEPS
    assert not torch.equal(res[0]["resid"], res[1]["resid"]) and res[0]["resid"].abs().max() > 0


BASE = ["--network", "LeNet", "--dataset", "MNIST", "--batch-size", "16", "--synthetic-size",
        "512", "--momentum", "0.9", "--lr", "0.05", "--eval-freq", "0", "--quiet",
        "--device", "cpu", "--log-interval", "1000", "--compress", "mx"]


def _train(rank, world, fmt, steps):
    import ewdml
    from ewdml.runtime import Trainer

    tr = Trainer(ewdml.parse_args(BASE + ["--mx-format", fmt, "--max-steps", str(steps)]))
    before = tr.flat.data.clone()
    losses = [float(tr.train_step()[0]) for _ in range(steps)]
    ex = tr.exchange
    return {"params": tr.flat.data.clone(), "before": before, "losses": losses,
            "payload_bytes": ex.last.payload_bytes,
            "layout_bytes": sum(lay.nbytes for lay in ex.codec.layouts),
            "ef_mode": ex.ef_mode, "resid_max": float(ex.resid.abs().max())}


@pytest.mark.parametrize("fmt", ["fp8", "fp4"])
def test_trainer_replicas_identical(tmp_path, fmt):
    res = run_world(_train, 2, tmp_path, args=(fmt, 4))
    assert torch.equal(res[0]["params"], res[1]["params"])
    for r in res:
        assert r["payload_bytes"] == r["layout_bytes"] > 0
        assert not torch.equal(r["params"], r["before"])
        assert all(l == l for l in r["losses"])
        assert r["ef_mode"] == "plain" and r["resid_max"] > 0
