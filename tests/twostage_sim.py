"""Shared by the two-stage sign all-reduce tests: prescribed gradients, a per-rank driver of the
real exchange, and a single-process simulation of all N ranks that calls the torch oracle
directly (no exchange, no codec dispatch, no communicator)."""
import torch

NUMELS = [20000, 8193, 31, 1, 100]  # bucket 0 = [20000] (3 chunks); bucket 1 = the rest (2 chunks)
BUCKET_BYTES = 64 << 10
TW = 2  # 1-bit Adam's dense warm-up steps


def make_flat(device="cpu"):
    from ewdml.parallel.flat import FlatModel

    gen = torch.Generator().manual_seed(7)
    params = [torch.nn.Parameter((torch.randn(n, generator=gen) * 0.1).to(device))
              for n in NUMELS]
    return FlatModel(params, bucket_bytes=BUCKET_BYTES, reverse=False)


def make_opt(flat, kind):
    from ewdml.optim.flat import FlatOnebitAdam, FlatSGD

    if kind == "sgd":  # lr = 2^-4, dampening 0: the step does not depend on fma contraction
        return FlatSGD(flat, lr=2.0 ** -4, momentum=0.5, weight_decay=0.0)
    return FlatOnebitAdam(flat, lr=2.0 ** -6, weight_decay=2.0 ** -5, freeze_step=TW)


def grad_of(step, rank, numel, device="cpu"):
    """Multiples of 1/16 in [-2, 2): any summation order over the ranks is exact in fp32, so the
    dense warm-up's all-reduce has one answer."""
    gen = torch.Generator().manual_seed(1000 * step + rank + 1)
    return (torch.randint(-32, 32, (numel,), generator=gen).float() / 16.0).to(device)


def state_of(flat, opt, ex=None):
    out = {"params": flat.data.clone().cpu()}
    for k in ("mom", "exp_avg", "exp_avg_sq"):
        if getattr(opt, k, None) is not None:
            out[k] = getattr(opt, k).clone().cpu()
    if ex is not None:
        out["resid"], out["sresid"] = ex.resid.clone().cpu(), ex.sresid.clone().cpu()
    return out


def run_rank(rank, world, kind, steps, device="cpu", comm=None):
    """One rank of the real thing: the exchange driven with the prescribed gradients."""
    from ewdml.compress import make_codec
    from ewdml.parallel.comm import Comm
    from ewdml.parallel.engine import GradientExchange
    from ewdml.parallel.twostage import TwoStageSignExchange

    comm = comm or Comm()
    flat = make_flat(device)
    opt = make_opt(flat, kind)
    ts = TwoStageSignExchange(flat, comm, make_codec("sign"), opt)
    dense = GradientExchange(flat, comm, make_codec("none"), opt, overlap=False,
                             side_stream=False) if kind == "onebit" else None
    stats = None
    for step in range(steps):
        ex = dense if (dense is not None and not opt.frozen) else ts
        flat.grad.copy_(grad_of(step, rank, flat.numel, device))
        ex.begin()
        ex.finish()
        if ex is ts:
            stats = ts.last
    out = state_of(flat, opt, ts)
    out["stats"] = (stats.payload_bytes, stats.wire_bytes_sent, stats.wire_bytes_recv,
                    stats.collectives)
    out["P"] = [t.P for t in ts.ts]
    out["shard_bytes"] = [[0 if lay is None else lay.nbytes for _, _, _, lay, _ in t.shards]
                          for t in ts.ts]
    return out


def simulate(world, kind, steps):
    """All ``world`` ranks in one process, straight from the oracle.  Returns the common replica
    state and every rank's two residuals (``sresid`` in the exchange's per-bucket slot layout)."""
    from ewdml.compress import Layout, oracle
    from ewdml.parallel.sharded import shard_plans

    N = world
    flat = make_flat()
    opt = make_opt(flat, kind)
    shards = []  # per bucket: [(s0, ln, plan | None, layout | None)]
    for b in flat.buckets:
        shards.append([(s0, ln, sp, None if sp is None else Layout.build("sign", sp))
                       for s0, ln, sp in shard_plans(b.plan, N, b.start)])
    slot = [(max(ln for _, ln, _, _ in sh) + 63) // 64 * 64 for sh in shards]
    soff = [sum(slot[:i]) for i in range(len(slot))]
    resid = [torch.zeros(flat.numel) for _ in range(N)]
    sresid = [torch.zeros(sum(slot)) for _ in range(N)]
    for step in range(steps):
        grads = [grad_of(step, r, flat.numel) for r in range(N)]
        if kind == "onebit" and not opt.frozen:  # dense Adam on the exact mean
            total = torch.zeros(flat.numel)
            for g in grads:
                total += g
            opt.step_range(0, flat.numel, total, 1.0 / N)
            opt.end_step()
            continue
        hp = opt.hparams()
        for b, sh in zip(flat.buckets, shards):
            for o, (s0, ln, sp, lay) in enumerate(sh):  # o: the shard and its owner
                if sp is None:
                    continue
                sl = slice(b.start + s0, b.start + s0 + ln)
                rows = []
                for r in range(N):  # stage 1: every worker's push of shard o
                    if kind == "onebit":
                        rows.append(oracle.encode_sign_momentum(
                            grads[r][sl], sp, lay, resid[r][sl], opt.exp_avg[sl], opt.betas[0],
                            opt.weight_decay, flat.data[sl]))
                    else:
                        rows.append(oracle.encode_sign(grads[r][sl], sp, lay, resid[r][sl]))
                # stage 2: the owner's average, server residual and second quantisation
                sv = sresid[o][soff[b.index]:soff[b.index] + ln]
                own = oracle.sign_reduce_encode(torch.stack(rows), sp, lay, 1.0 / N, sv)
                if kind == "onebit":
                    oracle.onebit_adam_apply(own[None], sp, lay, flat.data[sl], opt.exp_avg[sl],
                                             opt.exp_avg_sq[sl], 1.0, hp["lr_step"], hp["eps"])
                else:
                    g = oracle.decode_sum(own[None], sp, lay, 0, 1.0)
                    for off, n in zip(sp.offsets, sp.numels):
                        t = slice(b.start + s0 + off, b.start + s0 + off + n)
                        oracle.sgd_apply(flat.data[t], opt.mom[t], g[off:off + n], hp["lr"],
                                         hp["momentum"], hp["dampening"], hp["weight_decay"],
                                         hp["nesterov"], opt.first)
        opt.end_step()
    out = state_of(flat, opt)
    out["resid"], out["sresid"] = resid, sresid
    return out


def same_bits(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32),
                                              b.contiguous().view(torch.int32))
