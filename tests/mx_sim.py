"""Shared by the MX codec's exchange tests: LeNet-sized flat parameters, prescribed gradients, a
per-rank driver of the real all-gather exchange, and a single-process simulation of all N ranks
that calls the torch oracle directly (no exchange, no codec dispatch, no communicator)."""
import torch

# LeNet's tensors: conv1, conv2, fc1, fc2, each with its bias
NUMELS = [500, 20, 25000, 50, 400000, 500, 5000, 10]
BUCKET_BYTES = 256 << 10  # several buckets
HP = dict(lr=2.0 ** -4, momentum=0.9, dampening=0.0, weight_decay=2.0 ** -8, nesterov=False)


def make_flat(device="cpu"):
    from ewdml.parallel.flat import FlatModel

    gen = torch.Generator().manual_seed(7)
    params = [torch.nn.Parameter((torch.randn(n, generator=gen) * 0.1).to(device))
              for n in NUMELS]
    return FlatModel(params, bucket_bytes=BUCKET_BYTES, reverse=False)


def grad_of(step, rank, numel, device="cpu"):
    """Gaussian gradients whose scale differs by rank and by stretch of the buffer, so blocks of
    one step carry many different scale bytes and the rank order of the sum matters."""
    gen = torch.Generator().manual_seed(1000 * step + rank + 1)
    g = torch.randn(numel, generator=gen) * (0.01 * 3.0 ** rank)
    g *= torch.exp2(torch.randint(-6, 3, ((numel + 63) // 64,), generator=gen)
                    .float()).repeat_interleave(64)[:numel]
    return g.to(device)


def run_rank(rank, world, fmt, steps, device="cpu", comm=None):
    """One rank of the real thing: the exchange driven with the prescribed gradients."""
    from ewdml.compress import make_codec
    from ewdml.optim.flat import FlatSGD
    from ewdml.parallel.comm import Comm
    from ewdml.parallel.engine import GradientExchange, replica_fingerprint

    comm = comm or Comm()
    flat = make_flat(device)
    opt = FlatSGD(flat, **HP)
    ex = GradientExchange(flat, comm, make_codec("mx", fmt=fmt), opt, overlap=False,
                          error_feedback=True, side_stream=False)
    recv = []
    for step in range(steps):
        flat.grad.copy_(grad_of(step, rank, flat.numel, device))
        ex.begin()
        ex.finish()
        recv.append(ex.last.wire_bytes_recv)
    out = {"params": flat.data.clone().cpu(), "mom": opt.mom.clone().cpu(),
           "resid": ex.resid.clone().cpu(), "fp_params": replica_fingerprint(flat.data),
           "bytes_recv": recv, "payload": ex.last.payload_bytes, "ef_mode": ex.ef_mode,
           "layout_bytes": sum(lay.nbytes for lay in ex.codec.layouts),
           "lengths": [b.length for b in flat.buckets], "describe": ex.codec.describe()}
    ex.close()
    return out


def simulate(world, fmt, steps):
    """All ``world`` ranks in one process, straight from the oracle: the common parameters and
    momentum, and every rank's own residual."""
    from ewdml.compress import Layout, oracle

    bits = oracle.MX_NAMES[fmt]
    flat = make_flat()
    lays = [Layout.build("mx", b.plan, bits) for b in flat.buckets]
    mom = torch.zeros(flat.numel)
    resid = [torch.zeros(flat.numel) for _ in range(world)]
    for step in range(steps):
        grads = [grad_of(step, r, flat.numel) for r in range(world)]
        for b, lay in zip(flat.buckets, lays):
            sl = slice(b.start, b.start + b.length)
            rows = torch.stack([oracle.encode_mx(grads[r][sl], b.plan, lay, resid[r][sl])
                                for r in range(world)])
            g = oracle.decode_sum(rows, b.plan, lay, 0, 1.0 / world)
            for off, n in zip(b.plan.offsets, b.plan.numels):
                o = b.start + off
                oracle.sgd_apply(flat.data[o:o + n], mom[o:o + n], g[off:off + n], HP["lr"],
                                 HP["momentum"], HP["dampening"], HP["weight_decay"],
                                 HP["nesterov"], step == 0)
    return {"params": flat.data.clone(), "mom": mom, "resid": resid}


def same_bits(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32),
                                              b.contiguous().view(torch.int32))
