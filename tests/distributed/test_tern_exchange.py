"""The TernGrad codec through the all-gather exchange on CPU/Gloo, world 2: the trainer runs LeNet
with ``--compress tern`` with and without error feedback -- replicas stay bitwise identical and
every step sends the layouts' bytes -- and the real exchange, driven with prescribed gradients
over the codec's bucket of edge-case tensors, decodes step 1 to the mean that the independent
numpy simulation (tests/tern_sim.py) gives."""
import numpy as np
import pytest
import torch

from .. import tern_sim as sim
from .helpers import run_world

pytestmark = pytest.mark.slow

BASE = ["--network", "LeNet", "--dataset", "MNIST", "--batch-size", "16", "--synthetic-size",
        "512", "--momentum", "0.9", "--lr", "0.05", "--eval-freq", "0", "--quiet",
        "--device", "cpu", "--log-interval", "1000", "--compress", "tern"]
STEPS = 4


def _train(rank, world, flags):
    import ewdml
    from ewdml.runtime import Trainer

    tr = Trainer(ewdml.parse_args(BASE + list(flags) + ["--max-steps", str(STEPS)]))
    before = tr.flat.data.clone()
    ex = tr.exchange
    losses, sent = [], []
    for _ in range(STEPS):
        losses.append(float(tr.train_step()[0]))
        sent.append(ex.last.payload_bytes)
    return {"params": tr.flat.data.clone(), "before": before, "losses": losses, "sent": sent,
            "recv": ex.last.wire_bytes_recv,
            "layout_bytes": sum(lay.nbytes for lay in ex.codec.layouts),
            "formula": sum((4 * p.num_tensors + 15) // 16 * 16 + p.total_codes // 4
                           for p in ex.codec.plans),
            "describe": ex.codec.describe(), "ef_mode": ex.ef_mode,
            "resid_max": None if ex.resid is None else float(ex.resid.abs().max())}


@pytest.mark.parametrize("flags,describe,ef", [
    ([], "tern2b(c=2.5)", False),
    (["--error-feedback"], "tern2b(c=2.5)", True),
    (["--tern-clip", "0"], "tern2b", False),
], ids=["plain", "ef", "noclip"])
def test_trainer_replicas_identical(tmp_path, flags, describe, ef):
    res = run_world(_train, 2, tmp_path, args=(flags,))
    assert torch.equal(res[0]["params"].view(torch.int32), res[1]["params"].view(torch.int32))
    for r in res:
        assert r["describe"] == describe
        assert r["sent"] == [r["layout_bytes"]] * STEPS and r["layout_bytes"] > 0
        assert (r["formula"] + 15) // 16 * 16 >= r["layout_bytes"] >= r["formula"]
        assert r["recv"] == r["layout_bytes"]  # world 2: one other rank's payload
        assert not torch.equal(r["params"], r["before"])
        assert all(l == l for l in r["losses"])
        if ef:
            assert r["ef_mode"] == "plain" and r["resid_max"] > 0
        else:
            assert r["ef_mode"] is None and r["resid_max"] is None


def _exchange(rank, world, ef):
    """One step of the real exchange on zero parameters with lr 1 and no momentum: the parameters
    afterwards are minus the decoded mean, exactly."""
    from ewdml.compress import make_codec
    from ewdml.optim.flat import FlatSGD
    from ewdml.parallel.comm import Comm
    from ewdml.parallel.engine import GradientExchange
    from ewdml.parallel.flat import FlatModel

    comm = Comm()
    params = [torch.nn.Parameter(torch.zeros(n)) for n in sim.NUMELS]
    flat = FlatModel(params, bucket_bytes=4 << 20, reverse=False)
    opt = FlatSGD(flat, lr=1.0, momentum=0.0, dampening=0.0, weight_decay=0.0, nesterov=False)
    ex = GradientExchange(flat, comm, make_codec("tern", seed=9), opt, overlap=False,
                          error_feedback=ef, side_stream=False)
    if ef:
        ex.resid.copy_(torch.from_numpy(sim.bucket(20 + rank)) * 0.25)
    step = ex.step_idx + ex.seed_offset
    flat.grad.copy_(torch.from_numpy(sim.bucket(rank)))
    ex.begin()
    ex.finish()
    out = {"params": flat.data.clone(), "step": step, "offsets": list(flat.offsets),
           "buckets": [(b.start, b.length) for b in flat.buckets],
           "resid": None if ex.resid is None else ex.resid.clone()}
    ex.close()
    return out


@pytest.mark.parametrize("ef", [False, True], ids=["plain", "ef"])
def test_first_step_decodes_to_the_simulations_mean(tmp_path, ef):
    world = 2
    res = run_world(_exchange, world, tmp_path, args=(ef,))
    offs, length = sim.offsets()
    assert res[0]["offsets"] == offs and res[0]["buckets"] == [(0, length)]
    pays, resids = [], []
    for r in range(world):
        r0 = (sim.bucket(20 + r) * np.float32(0.25)).astype(np.float32) if ef else None
        key = sim.stream_key(9, res[r]["step"], r)
        pay, _, new = sim.encode(sim.bucket(r), sim.NUMELS, offs, 0, 2.5, key, r0)
        pays.append(pay)
        resids.append(new)
    mean = sim.decode_mean(pays, sim.NUMELS, offs, length, 1.0 / world)
    for r in range(world):
        got = res[r]["params"].numpy()
        assert np.array_equal((-got).view(np.int32) & 0x7FFFFFFF, mean.view(np.int32) & 0x7FFFFFFF)
        assert np.array_equal(np.signbit(got) & (got != 0), (mean > 0))
        if ef:
            assert np.array_equal(res[r]["resid"].numpy().view(np.int32),
                                  resids[r].view(np.int32))
    assert np.abs(mean).max() > 0
