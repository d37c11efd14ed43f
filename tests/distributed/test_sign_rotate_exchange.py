"""The Hadamard-rotated sign codec through the all-gather exchange on CPU/Gloo: 2 and 3 ranks run
the real exchange over LeNet-sized buckets with prescribed gradients.  Replicas stay bitwise
identical and equal a single-process simulation that calls the oracle directly: every rank's
encode with its own residual, the rows summed in rank order, one decode, one SGD step."""
import pytest
import torch

from ..lion_sim import make_flat, same_bits
from .helpers import run_world

pytestmark = pytest.mark.slow

STEPS = 3
SEED = 5
HP = dict(lr=2.0 ** -4, momentum=0.9, dampening=0.0, weight_decay=0.0, nesterov=False)


def _grad(step, rank, numel):
    gen = torch.Generator().manual_seed(1000 * step + rank + 1)
    g = torch.randn(numel, generator=gen) ** 3  # heavy-tailed: what the rotation is for
    return g * (4.0 ** rank)  # the rank order of the fp32 sum matters


def _rank(rank, world):
    from ewdml.compress import make_codec
    from ewdml.optim import make_optimizer
    from ewdml.parallel.comm import Comm
    from ewdml.parallel.engine import GradientExchange

    flat = make_flat()
    opt = make_optimizer("sgd", flat, lr=HP["lr"], momentum=HP["momentum"])
    codec = make_codec("sign", rotate="hadamard", seed=SEED)
    ex = GradientExchange(flat, Comm(), codec, opt, overlap=False, side_stream=False,
                          error_feedback=True)
    recv = []
    for step in range(STEPS):
        flat.grad.copy_(_grad(step, rank, flat.numel))
        ex.begin()
        ex.finish()
        recv.append(ex.last.wire_bytes_recv)
    out = {"params": flat.data.clone(), "mom": opt.mom.clone(), "resid": ex.resid.clone(),
           "bytes_recv": recv, "payload": ex.last.payload_bytes, "buckets": len(flat.buckets),
           "layout": sum(lay.nbytes for lay in codec.layouts), "label": codec.describe()}
    ex.close()
    return out


def _simulate(world):
    from ewdml.compress import Layout, oracle

    flat = make_flat()
    lays = [Layout.build("sign", b.plan) for b in flat.buckets]
    mom = torch.zeros(flat.numel)
    resid = [torch.zeros(flat.numel) for _ in range(world)]
    for step in range(STEPS):
        grads = [_grad(step, r, flat.numel) for r in range(world)]
        for b, lay in zip(flat.buckets, lays):
            sl = slice(b.start, b.start + b.length)
            key = oracle.hsign_rot_key(SEED, b.index)
            rows = torch.stack([oracle.encode_sign(grads[r][sl], b.plan, lay, resid[r][sl], key)
                                for r in range(world)])
            g = oracle.decode_sum(rows, b.plan, lay, 0, 1.0 / world, key)
            p, m = flat.data[sl], mom[sl]
            for off, n in zip(b.plan.offsets, b.plan.numels):
                oracle.sgd_apply(p[off:off + n], m[off:off + n], g[off:off + n], first=step == 0,
                                 **HP)
    return {"params": flat.data.clone(), "mom": mom, "resid": resid}


@pytest.mark.parametrize("world", [2, 3])
def test_replicas_equal_the_oracle_simulation(tmp_path, world):
    res = run_world(_rank, world, tmp_path)
    sim = _simulate(world)
    r0 = res[0]
    assert r0["buckets"] > 1 and r0["label"] == "sign1b-h"
    for r, out in enumerate(res):
        assert same_bits(out["params"], r0["params"])  # replicas: bitwise identical
        assert same_bits(out["params"], sim["params"]), f"rank {r}: parameters"
        assert same_bits(out["mom"], sim["mom"]), f"rank {r}: momentum"
        assert same_bits(out["resid"], sim["resid"][r]), f"rank {r}: residual"
        assert out["payload"] == out["layout"] > 0
        assert out["bytes_recv"] == [(world - 1) * out["payload"]] * STEPS
    assert not torch.equal(res[0]["resid"], res[1]["resid"])  # per-rank state
