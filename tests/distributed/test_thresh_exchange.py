"""The threshold-search sparsifier through the all-gather exchange on CPU/Gloo, worlds 2 and 3: the
real exchange, driven for three steps with prescribed gradients over the codec's bucket of
edge-case tensors and with error feedback, leaves the parameters and every rank's residual that the
independent numpy simulation (tests/thresh_sim.py) gives; replicas stay bitwise identical and
every step receives (N - 1) payloads of the layout's bytes."""
import numpy as np
import pytest
import torch

from .. import thresh_sim as sim
from .helpers import run_world

pytestmark = pytest.mark.slow

STEPS = 3


def _grad(step, rank):
    return sim.bucket(10 * step + rank)


def _exchange(rank, world):
    """Three steps on zero parameters with lr 1 and no momentum: every step subtracts the decoded
    mean, exactly."""
    from ewdml.compress import make_codec
    from ewdml.optim.flat import FlatSGD
    from ewdml.parallel.comm import Comm
    from ewdml.parallel.engine import GradientExchange
    from ewdml.parallel.flat import FlatModel

    comm = Comm()
    params = [torch.nn.Parameter(torch.zeros(n)) for n in sim.NUMELS]
    flat = FlatModel(params, bucket_bytes=4 << 20, reverse=False)
    opt = FlatSGD(flat, lr=1.0, momentum=0.0, dampening=0.0, weight_decay=0.0, nesterov=False)
    codec = make_codec("thresh", ratio=sim.RATIO, dense_below=sim.DENSE_BELOW, seed=9)
    ex = GradientExchange(flat, comm, codec, opt, overlap=False, error_feedback=True,
                          side_stream=False)
    out = {"offsets": list(flat.offsets), "buckets": [(b.start, b.length) for b in flat.buckets],
           "payload_bytes": codec.payload_bytes(0), "describe": codec.describe(),
           "ef_mode": ex.ef_mode, "params": [], "resid": [], "sent": [], "recv": []}
    for step in range(STEPS):
        flat.grad.copy_(torch.from_numpy(_grad(step, rank)))
        ex.begin()
        ex.finish()
        out["params"].append(flat.data.clone())
        out["resid"].append(ex.resid.clone())
        out["sent"].append(ex.last.payload_bytes)
        out["recv"].append(ex.last.wire_bytes_recv)
    ex.close()
    return out


@pytest.mark.parametrize("world", [2, 3])
def test_three_steps_against_the_simulation(tmp_path, world):
    res = run_world(_exchange, world, tmp_path)
    offs, length = sim.offsets()
    nbytes = sim.layout(sim.NUMELS, offs)[2]
    for r in res:
        assert r["offsets"] == offs and r["buckets"] == [(0, length)]
        assert r["describe"] == "thresh-k0.01" and r["ef_mode"] == "plain"
        assert r["payload_bytes"] == nbytes
        assert r["sent"] == [nbytes] * STEPS and r["recv"] == [(world - 1) * nbytes] * STEPS
    resid = [np.zeros(length, dtype=np.float32) for _ in range(world)]
    p = np.zeros(length, dtype=np.float32)
    for step in range(STEPS):
        pays = []
        for r in range(world):
            pay, _, resid[r] = sim.encode(_grad(step, r), sim.NUMELS, offs, resid[r])
            pays.append(pay)
        mean = sim.decode_mean(pays, sim.NUMELS, offs, length, 1.0 / world)
        with np.errstate(invalid="ignore"):
            p = (p - mean).astype(np.float32)
        for r in range(world):
            got = res[r]["params"][step]
            assert torch.equal(got.view(torch.int32), res[0]["params"][step].view(torch.int32))
            assert np.array_equal(got.numpy().view(np.int32), p.view(np.int32)), \
                f"step {step}, rank {r}: parameters"
            assert np.array_equal(res[r]["resid"][step].numpy().view(np.int32),
                                  resid[r].view(np.int32)), f"step {step}, rank {r}: residual"
    assert np.isfinite(p).sum() > 0.9 * length and np.abs(np.nan_to_num(p)).max() > 0
