"""Shared by the count-sketch tests: an independent numpy simulation of the whole exchange
(integer hashing from scratch, the stated summation order, the compare-exchange medians, the
top-k rule, the gather and the SGD step), the test plans, and a per-rank driver of the real
exchange with prescribed gradients.

Nothing here imports the oracle: the simulation restates the semantics of ``compress/oracle.py
sketch_*`` from their description."""
import math

import numpy as np
import torch

CHUNK = 8192
GROUP = 64  # chunks per summation group
ALIGN = 64
M32 = 0xFFFFFFFF
SHIFT_TAG = 0x534B5348
SIGN_TAG = 0x534B5347
f32 = np.float32


# ---- hashing from scratch ---------------------------------------------------------------------
def mix32(x: int) -> int:
    x &= M32
    x ^= x >> 16
    x = (x * 0x7FEB352D) & M32
    x ^= x >> 15
    x = (x * 0x846CA68B) & M32
    x ^= x >> 16
    return x


def mix32_np(x: np.ndarray) -> np.ndarray:
    x = x.astype(np.uint64) & np.uint64(M32)
    x ^= x >> np.uint64(16)
    x = (x * np.uint64(0x7FEB352D)) & np.uint64(M32)
    x ^= x >> np.uint64(15)
    x = (x * np.uint64(0x846CA68B)) & np.uint64(M32)
    x ^= x >> np.uint64(16)
    return x


def stream_key(seed: int, step: int, rank: int) -> int:
    k = mix32((step * 0x9E3779B9 + rank * 0x85EBCA6B + 0x632BE59B) & M32)
    return mix32((seed & M32) ^ k)


# ---- one bucket ---------------------------------------------------------------------------------
class SimBucket:
    """Tensors ``numels`` at ``offsets`` of a bucket; ``k = numel`` where ``numel <= dense_below``
    else ``max(1, int(numel * ratio))``."""

    def __init__(self, numels, offsets, ratio, dense_below, bucket_offset, length, rows, width,
                 seed, bucket):
        self.numels, self.offsets = list(numels), list(offsets)
        self.bucket_offset, self.length, self.rows = bucket_offset, length, rows
        self.ks = [n if n <= dense_below else max(1, int(n * ratio)) for n in numels]
        self.dense = [k == n for k, n in zip(self.ks, numels)]
        self.K = sum(k for k, d in zip(self.ks, self.dense) if not d)
        self.dense_elems = sum(n for n, d in zip(numels, self.dense) if d)
        self.W = CHUNK * max(1, math.ceil(width * self.K / CHUNK))
        self.sk_key = stream_key(seed, bucket, SHIFT_TAG)
        self.sg_key = stream_key(seed, bucket, SIGN_TAG)
        self.chunks = []  # (tensor, start, len), dense tensors' chunks included: they count in c
        for t, (n, off) in enumerate(zip(numels, offsets)):
            for s in range(0, n, CHUNK):
                self.chunks.append((t, off + s, min(CHUNK, n - s)))
        self.shifts = [[(mix32((c * 8 + j) ^ self.sk_key) * self.W) >> 32
                        for c in range(len(self.chunks))] for j in range(rows)]

    def payload_bytes(self):
        return 4 * (self.rows * self.W + self.K + self.dense_elems)

    def signs(self, start, ln):
        """uint64 hash per element of a chunk: bit j is the sign in row j."""
        gidx = (self.bucket_offset + start + np.arange(ln, dtype=np.uint64)) & np.uint64(M32)
        return mix32_np(gidx ^ np.uint64(self.sg_key))

    @staticmethod
    def signed(x, h, j):
        return np.where(((h >> np.uint64(j)) & np.uint64(1)).astype(bool), -x, x)

    def stage(self, g, resid):
        for t, (n, off) in enumerate(zip(self.numels, self.offsets)):
            if not self.dense[t]:
                resid[off:off + n] = g[off:off + n] + resid[off:off + n]

    def table(self, acc):
        W = self.W
        T = np.zeros((self.rows, W), dtype=f32)
        for j in range(self.rows):
            for g0 in range(0, len(self.chunks), GROUP):
                part = np.zeros(W, dtype=f32)
                for c in range(g0, min(g0 + GROUP, len(self.chunks))):
                    t, start, ln = self.chunks[c]
                    if self.dense[t]:
                        continue
                    v = self.signed(acc[start:start + ln], self.signs(start, ln), j)
                    cols = (np.arange(ln) + self.shifts[j][c]) % W  # distinct: ln <= CHUNK <= W
                    part[cols] = part[cols] + v
                T[j] = T[j] + part
        return T.reshape(-1)

    @staticmethod
    def median(v):
        v = list(v)
        net = {1: (), 3: ((0, 1), (1, 2), (0, 1)),
               5: ((0, 1), (3, 4), (2, 4), (2, 3), (1, 4), (0, 3), (0, 2), (1, 3), (1, 2))}[len(v)]
        for a, b in net:
            s = v[b] < v[a]
            v[a], v[b] = np.where(s, v[b], v[a]), np.where(s, v[a], v[b])
        return v[len(v) // 2]

    def estimate(self, table):
        W = self.W
        T = table.reshape(self.rows, W)
        est = np.zeros(self.length, dtype=f32)
        for c, (t, start, ln) in enumerate(self.chunks):
            if self.dense[t]:
                continue
            h = self.signs(start, ln)
            est[start:start + ln] = self.median(
                [self.signed(T[j][(np.arange(ln) + self.shifts[j][c]) % W], h, j)
                 for j in range(self.rows)])
        return est

    def select(self, est):
        """Bucket positions of the selected elements in payload order: per tensor the k largest
        |est|, ties to the lowest index, sorted by index."""
        pos = []
        for n, off, k in zip(self.numels, self.offsets, self.ks):
            key = (est[off:off + n].view(np.uint32) & np.uint32(0x7FFFFFFF)).astype(np.int64)
            sel = np.sort(np.argsort(-key, kind="stable")[:k])
            pos.append(off + sel)
        return np.concatenate(pos)

    def gather(self, pos, g, resid):
        src = resid.copy()
        for t, (n, off) in enumerate(zip(self.numels, self.offsets)):
            if self.dense[t]:
                src[off:off + n] = g[off:off + n]
        vals = src[pos].copy()
        resid[pos] = 0.0
        return vals

    def decoded(self, pos, vals, inv_n):
        ghat = np.zeros(self.length, dtype=f32)
        ghat[pos] = (f32(0.0) + vals) * f32(inv_n)
        return ghat

    def sgd(self, param, mom, ghat, lr, momentum, first):
        for n, off in zip(self.numels, self.offsets):
            sl = slice(off, off + n)
            if first:
                mom[sl] = ghat[sl]
            else:
                mom[sl] = mom[sl] * f32(momentum) + ghat[sl]
            param[sl] = param[sl] + f32(-lr) * mom[sl]

    def step(self, grads, resids, param, mom, lr, momentum, first):
        """One exchange of this bucket for all ranks (sums in rank order).  ``grads`` / ``resids``:
        per rank bucket views (residuals updated in place); returns the intermediate results."""
        N = len(grads)
        for g, r in zip(grads, resids):
            self.stage(g, r)
        tables = [self.table(r) for r in resids]
        T = tables[0].copy()
        for x in tables[1:]:
            T = T + x
        est = self.estimate(T)
        pos = self.select(est)
        vals_r = [self.gather(pos, g, r) for g, r in zip(grads, resids)]
        vals = vals_r[0].copy()
        for x in vals_r[1:]:
            vals = vals + x
        ghat = self.decoded(pos, vals, 1.0 / N)
        self.sgd(param, mom, ghat, lr, momentum, first)
        return {"tables": tables, "table": T, "est": est, "pos": pos, "vals_r": vals_r,
                "vals": vals, "ghat": ghat}


# ---- test plans ---------------------------------------------------------------------------------
# several chunks and a tail | exactly 64 | dense (k == numel through dense_below) | one element
# (k = 1 = numel: dense) | more chunks than one summation group, with a tail
NUMELS = [3 * CHUNK + 17, 64, 40, 1, 66 * CHUNK + 5]
RATIO, DENSE_BELOW, SEED = 0.01, 40, 5


def layout(numels):
    offs, total = [], 0
    for n in numels:
        offs.append(total)
        total += (n + ALIGN - 1) // ALIGN * ALIGN
    return offs, total


def make_plans(rows, width, numels=NUMELS, ratio=RATIO, dense_below=DENSE_BELOW,
               bucket_offset=1 << 20, edges=True):
    """(SketchPlan, Layout, SimBucket) over the same tensors with the same hand-set shifts: chunk
    0 of row 0 at W - 1 (wraps after one element) and the 17-element tail chunk of tensor 0 at
    W - 17 (ends on the last column, no wrap)."""
    from ewdml.compress import oracle
    from ewdml.compress.plan import BucketPlan, Layout, SketchPlan

    offs, total = layout(numels)
    bp = BucketPlan(list(numels), offs, ratio, bucket_offset, total, dense_below)
    sp = SketchPlan(bp, rows, width, *oracle.sketch_keys(SEED, 0))
    sim = SimBucket(numels, offs, ratio, dense_below, bucket_offset, total, rows, width, SEED, 0)
    if edges:
        for c, o in ((0, sp.W - 1), (3, sp.W - 17)):
            sp.set_shift(0, c, o)
            sim.shifts[0][c] = o
    return sp, Layout.build("topk", bp), sim


def same_bits(a, b):
    a = torch.as_tensor(a).detach().cpu().contiguous()
    b = torch.as_tensor(b).detach().cpu().contiguous()
    return a.shape == b.shape and torch.equal(a.view(torch.int32), b.view(torch.int32))


def grad_of(step, rank, n):
    gen = torch.Generator().manual_seed(1000 * step + rank + 1)
    return torch.randn(n, generator=gen)


# ---- the real exchange, driven with prescribed gradients ---------------------------------------
SHAPES = [(40, 50), (10,), (3 * CHUNK + 17,), (7,), (64,)]
BUCKET_BYTES = 16 << 10  # two buckets: [2000, 10] | [24593, 7, 64]
EX = dict(ratio=0.05, dense_below=10, rows=3, width=2.0, seed=3)
LR, MOMENTUM = 2.0 ** -4, 0.5  # powers of two: the step does not depend on fma contraction


def make_flat(device="cpu"):
    from ewdml.parallel.flat import FlatModel

    gen = torch.Generator().manual_seed(7)
    params = [torch.nn.Parameter((torch.randn(*s, generator=gen) * 0.1).to(device))
              for s in SHAPES]
    return FlatModel(params, bucket_bytes=BUCKET_BYTES, reverse=False)


def run_rank(rank, world, steps, device="cpu", optimizer="sgd"):
    from ewdml.compress import make_codec
    from ewdml.optim.flat import FlatSGD, make_optimizer
    from ewdml.parallel.comm import Comm
    from ewdml.parallel.sketch import SketchExchange

    flat = make_flat(device)
    if optimizer == "sgd":
        opt = FlatSGD(flat, lr=LR, momentum=MOMENTUM, weight_decay=0.0)
    else:
        opt = make_optimizer(optimizer, flat, lr=1e-3)
    ex = SketchExchange(flat, Comm(), make_codec("sketch", **EX), opt)
    counts = []
    for step in range(steps):
        flat.grad.copy_(grad_of(step, rank, flat.numel).to(device))
        ex.begin()
        ex.finish()
        from ewdml.compress import oracle

        counts = [[int(c) for c in torch.bincount(torch.searchsorted(
            torch.tensor(p.offsets), oracle._decoded_entries(
                ex.payload[bi].cpu(), p, ex.codec.layouts[bi], 0)[0], right=True) - 1,
            minlength=p.num_tensors)] for bi, p in enumerate(ex.codec.plans)]
    st = ex.last
    return {"params": flat.data.clone().cpu(), "resid": ex.resid.clone().cpu(),
            "mom": opt.mom.clone().cpu() if getattr(opt, "mom", None) is not None else None,
            "stats": (st.payload_bytes, st.wire_bytes_sent, st.wire_bytes_recv, st.collectives),
            "floats": [t.payload_floats for t in ex.sk], "ks": [p.ks for p in ex.codec.plans],
            "counts": counts, "buckets": len(flat.buckets)}


def simulate(world, steps):
    """All ``world`` ranks in numpy.  Returns the common parameters / momentum and every rank's
    residual."""
    flat = make_flat()
    param = flat.data.detach().numpy().copy()
    mom = np.zeros_like(param)
    resid = [np.zeros_like(param) for _ in range(world)]
    sims = [SimBucket(b.plan.numels, b.plan.offsets, EX["ratio"], EX["dense_below"], b.start,
                      b.length, EX["rows"], EX["width"], EX["seed"], b.index)
            for b in flat.buckets]
    for step in range(steps):
        grads = [grad_of(step, r, flat.numel).numpy() for r in range(world)]
        for b, sb in zip(flat.buckets, sims):
            sl = slice(b.start, b.start + b.length)
            sb.step([g[sl] for g in grads], [r[sl] for r in resid], param[sl], mom[sl], LR,
                    MOMENTUM, step == 0)
    return {"params": torch.from_numpy(param), "mom": torch.from_numpy(mom),
            "resid": [torch.from_numpy(r) for r in resid]}
