"""Shared by the PowerSGD tests: a bucket plan from tensor shapes, the 64-element aligned layout of
the flat buffer, the error metric, prescribed gradients, a per-rank driver of the real exchange
and a single-process simulation of all N ranks straight from the torch oracle."""
import torch

ALIGN = 64
# two buckets under BUCKET_BYTES: [40, 50] + [10] | [30, 3, 3, 3] + [7] + [5, 6] (too small: dense)
SHAPES = [(40, 50), (10,), (30, 3, 3, 3), (7,), (5, 6)]
BUCKET_BYTES = 8 << 10
RANK = 2


def numel(shape):
    n = 1
    for v in shape:
        n *= int(v)
    return n


def make_plan(shapes, rank, bucket_offset=0):
    """(LowRankPlan, bucket length) of the tensors ``shapes`` laid out as ``FlatModel`` does."""
    from ewdml.compress.plan import BucketPlan, LowRankPlan

    offs, total = [], 0
    for s in shapes:
        offs.append(total)
        total += (numel(s) + ALIGN - 1) // ALIGN * ALIGN
    bp = BucketPlan([numel(s) for s in shapes], offs, 1.0, bucket_offset, total)
    return LowRankPlan(bp, shapes, rank), total


def rel(a, b):
    """``_rel`` of tests/kernels/test_conv_f32.py."""
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return float((a - b).norm() / (b.norm() + 1e-30))


def same_bits(a, b):
    a, b = a.detach().cpu().contiguous(), b.detach().cpu().contiguous()
    return a.shape == b.shape and torch.equal(a.view(torch.int32), b.view(torch.int32))


def make_flat(device="cpu"):
    from ewdml.parallel.flat import FlatModel

    gen = torch.Generator().manual_seed(7)
    params = [torch.nn.Parameter((torch.randn(*s, generator=gen) * 0.1).to(device))
              for s in SHAPES]
    return FlatModel(params, bucket_bytes=BUCKET_BYTES, reverse=False)


def make_opt(flat):
    from ewdml.optim.flat import FlatSGD

    # powers of two: the step does not depend on fma contraction
    return FlatSGD(flat, lr=2.0 ** -4, momentum=0.5, weight_decay=0.0)


def grad_of(step, rank, n, device="cpu"):
    gen = torch.Generator().manual_seed(1000 * step + rank + 1)
    return torch.randn(n, generator=gen).to(device)


def run_rank(rank, world, steps, device="cpu"):
    """One rank of the real thing: the exchange driven with the prescribed gradients."""
    from ewdml.compress import make_codec
    from ewdml.parallel.comm import Comm
    from ewdml.parallel.powersgd import PowerSGDExchange

    flat = make_flat(device)
    opt = make_opt(flat)
    ex = PowerSGDExchange(flat, Comm(), make_codec("powersgd", rank=RANK, seed=3), opt)
    for step in range(steps):
        flat.grad.copy_(grad_of(step, rank, flat.numel, device))
        ex.begin()
        ex.finish()
    st = ex.last
    return {"params": flat.data.clone().cpu(), "mom": opt.mom.clone().cpu(),
            "resid": ex.resid.clone().cpu(),
            "q": [ex.q_view(bi)[:t.q_floats].clone().cpu() for bi, t in enumerate(ex.lr_plans)],
            "stats": (st.payload_bytes, st.wire_bytes_sent, st.wire_bytes_recv, st.collectives),
            "floats": [(t.p_floats, t.q_floats) for t in ex.lr_plans],
            "buckets": len(flat.buckets)}


def simulate(world, steps, dtype=torch.float32):
    """All ``world`` ranks in one process, straight from the oracle in ``dtype``: factors summed
    in rank order.  Returns the common parameters / momentum / q and every rank's residual."""
    from ewdml.compress import oracle
    from ewdml.compress.plan import LowRankPlan

    flat = make_flat()
    N, inv = world, 1.0 / world
    plans = [LowRankPlan(b.plan, [tuple(p.shape) for p in b.params], RANK) for b in flat.buckets]
    data, mom = flat.data.clone().to(dtype), torch.zeros(flat.numel, dtype=dtype)
    resid = [torch.zeros(flat.numel, dtype=dtype) for _ in range(N)]
    q = [oracle.powersgd_init_q(t, 3, bi).to(dtype) for bi, t in enumerate(plans)]
    hp = dict(lr=2.0 ** -4, momentum=0.5, dampening=0.0, weight_decay=0.0, nesterov=False)
    for step in range(steps):
        grads = [grad_of(step, r, flat.numel).to(dtype) for r in range(N)]
        for b, t in zip(flat.buckets, plans):
            sl = slice(b.start, b.start + b.length)
            ps = [oracle.powersgd_project(grads[r][sl], resid[r][sl], q[b.index], t, dtype)
                  for r in range(N)]
            p = ps[0].clone()
            for x in ps[1:]:
                p += x
            oracle.powersgd_orthogonalize(p, t, inv, dtype)
            qs = [oracle.powersgd_backproject(resid[r][sl], p, t, dtype) for r in range(N)]
            qsum = qs[0].clone()
            for x in qs[1:]:
                qsum += x
            for r in range(N):  # every rank reconstructs; rank 0's copy takes the step
                qa = oracle.powersgd_reconstruct_apply(
                    resid[r][sl], p, qsum, t, inv, data[sl] if r == 0 else None,
                    mom[sl] if r == 0 else None, hp, step == 0, dtype=dtype)
            q[b.index] = qa
    return {"params": data, "mom": mom, "resid": resid, "q": q}
