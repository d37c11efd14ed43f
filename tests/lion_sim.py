"""Shared by the Distributed Lion tests: LeNet-sized flat parameters, prescribed gradients, a
per-rank driver of the real vote exchange, and a single-process simulation of all N ranks that
calls the torch oracle directly (no exchange, no codec dispatch, no communicator)."""
import torch

# LeNet's tensors: conv1, conv2, fc1, fc2, each with its bias
NUMELS = [500, 20, 25000, 50, 400000, 500, 5000, 10]
BUCKET_BYTES = 256 << 10  # several buckets
LR, BETAS, WD = 2.0 ** -10, (0.9, 0.99), 2.0 ** -5


def make_flat(device="cpu"):
    from ewdml.parallel.flat import FlatModel

    gen = torch.Generator().manual_seed(7)
    params = [torch.nn.Parameter((torch.randn(n, generator=gen) * 0.1).to(device))
              for n in NUMELS]
    return FlatModel(params, bucket_bytes=BUCKET_BYTES, reverse=False)


def make_opt(flat):
    from ewdml.optim.flat import FlatLion

    return FlatLion(flat, lr=LR, betas=BETAS, weight_decay=WD)


def grad_of(step, rank, numel, device="cpu"):
    """Multiples of 1/16 in [-2, 2): one value in 64 is an exact zero, so the first step (zero
    momentum) dithers, and later steps do wherever every gradient so far was zero."""
    gen = torch.Generator().manual_seed(1000 * step + rank + 1)
    g = torch.randint(-32, 32, (numel,), generator=gen).float() / 16.0
    g[::97] = 0.0  # coordinates whose gradient is zero on every rank and step
    return g.to(device)


def run_rank(rank, world, aggregate, steps, device="cpu", comm=None):
    """One rank of the real thing: the exchange driven with the prescribed gradients."""
    from ewdml.compress import make_codec
    from ewdml.parallel.comm import Comm
    from ewdml.parallel.engine import GradientExchange, replica_fingerprint

    comm = comm or Comm()
    flat = make_flat(device)
    opt = make_opt(flat)
    ex = GradientExchange(flat, comm, make_codec("vote", aggregate=aggregate), opt, overlap=False,
                          side_stream=False)
    recv = []
    for step in range(steps):
        flat.grad.copy_(grad_of(step, rank, flat.numel, device))
        ex.begin()
        ex.finish()
        recv.append(ex.last.wire_bytes_recv)
    out = {"params": flat.data.clone().cpu(), "exp_avg": opt.exp_avg.clone().cpu(),
           "fp_params": replica_fingerprint(flat.data), "fp_exp_avg": replica_fingerprint(opt.exp_avg),
           "bytes_recv": recv, "payload": ex.last.payload_bytes,
           "chunks": sum(b.plan.num_chunks for b in flat.buckets), "buckets": len(flat.buckets)}
    ex.close()
    return out


def simulate(world, aggregate, steps):
    """All ``world`` ranks in one process, straight from the oracle: the common parameters and
    every rank's own momentum."""
    from ewdml.compress import Layout, oracle

    flat = make_flat()
    lays = [Layout.build("vote", b.plan) for b in flat.buckets]
    moms = [torch.zeros(flat.numel) for _ in range(world)]
    for step in range(steps):
        grads = [grad_of(step, r, flat.numel) for r in range(world)]
        for b, lay in zip(flat.buckets, lays):
            sl = slice(b.start, b.start + b.length)
            rows = torch.stack([oracle.encode_vote(grads[r][sl], b.plan, lay, moms[r][sl],
                                                   BETAS[0], BETAS[1], step + 1, r)
                                for r in range(world)])
            oracle.vote_apply(rows, b.plan, lay, flat.data[sl], LR, WD, aggregate, 1.0 / world)
    return {"params": flat.data.clone(), "exp_avg": moms}


def same_bits(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32),
                                              b.contiguous().view(torch.int32))
