"""The sign codec through the all-gather exchange on CPU/Gloo: 2 and 3 ranks train LeNet for a few
steps with ``--compress sign`` (error feedback on by default) and stay bitwise identical."""
import pytest
import torch

from .helpers import run_world

pytestmark = pytest.mark.slow

BASE = ["--network", "LeNet", "--dataset", "MNIST", "--batch-size", "16", "--synthetic-size",
        "512", "--momentum", "0.9", "--lr", "0.05", "--eval-freq", "0", "--quiet",
        "--device", "cpu", "--log-interval", "1000", "--compress", "sign"]


def _train(rank, world, steps):
    import ewdml
    from ewdml.runtime import Trainer

    cfg = ewdml.parse_args(BASE + ["--max-steps", str(steps)])
    tr = Trainer(cfg)
    before = tr.flat.data.clone()
    losses = []
    for _ in range(steps):
        loss, _ = tr.train_step()
        losses.append(float(loss))
    ex = tr.exchange
    return {"params": tr.flat.data.clone(), "before": before, "losses": losses,
            "payload_bytes": ex.last.payload_bytes, "bytes_recv": ex.last.wire_bytes_recv,
            "layout_bytes": sum(lay.nbytes for lay in ex.codec.layouts),
            "ef_mode": ex.ef_mode, "resid_max": float(ex.resid.abs().max())}


@pytest.mark.parametrize("world", [2, 3])
def test_sign_replicas_identical(tmp_path, world):
    res = run_world(_train, world, tmp_path, args=(6,))
    for r in res[1:]:
        assert torch.equal(r["params"], res[0]["params"])
    for r in res:
        assert r["payload_bytes"] == r["layout_bytes"] > 0
        assert r["bytes_recv"] == (world - 1) * r["layout_bytes"]
        assert not torch.equal(r["params"], r["before"])
        assert all(l == l for l in r["losses"])
        assert r["ef_mode"] == "plain" and r["resid_max"] > 0
