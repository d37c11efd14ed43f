"""A second opinion for the IntSGD oracle (compress/oracle.py encode_intsgd / intsgd_apply /
intsgd_alpha): the same codec, receive side and scale rule written again in plain numpy -- its own
counter RNG, its own chunk rows, its own summation tree and its own SGD -- sharing no code with the
oracle.  Also the fixed bucket of edge-case tensors that the codec's CPU and GPU tests share, and a
small N-rank training simulation for the exchange tests."""
import math

import numpy as np

F = np.float32
CHUNK = 8192
M32 = 0xFFFFFFFF
BETA, EPS2 = 0.9, 1e-16

# the one-element tensor, a 16-byte vector edge on both sides, a wave, the chunk edge on both sides
# and a three-chunk tensor; with the pads between them the smallest shapes that cross a 16-byte
# store, a wave, a chunk row and a bucket pad
NUMELS = [1, 15, 16, 17, 1000, 8191, 8192, 8193, 20000]
BUCKET_OFFSET = 4096
# tensors overwritten by bucket(): all zeros | exact integers after scaling | beyond +-q / alpha,
# a NaN and both infinities
ZERO_T, INT_T, WILD_T = 3, 4, 5
ALPHA = 64.0  # the power-of-two scale the integer tensor is built for
WORLDS = {1: 127, 2: 63, 3: 42, 8: 15, 127: 1}  # world -> q


def q_of(world):
    return 127 // world


def offsets(numels=NUMELS):
    """Tensors packed at multiples of 64 elements (parallel/flat.py): (offsets, bucket length)."""
    offs, o = [], 0
    for n in numels:
        offs.append(o)
        o += (n + 63) // 64 * 64
    return offs, o


def bucket(seed=0, q=15, numels=NUMELS, alpha=ALPHA):
    """fp32 bucket of fixed-seed normal draws around 0.3 q / alpha (0 between the tensors) with
    one all-zero tensor, one of exact multiples of 1 / alpha (both signs, some beyond q) and one
    that holds values beyond +-q / alpha, a NaN, +inf and -inf."""
    offs, length = offsets(numels)
    rs = np.random.RandomState(4321 + seed)
    g = np.zeros(length, dtype=F)
    for t, (o, n) in enumerate(zip(offs, numels)):
        g[o:o + n] = (rs.standard_normal(n) * (0.3 * q / alpha)).astype(F)
    if numels is NUMELS:
        o, n = offs[ZERO_T], numels[ZERO_T]
        g[o:o + n] = 0.0
        o, n = offs[INT_T], numels[INT_T]
        k = rs.randint(-q - 2, q + 3, size=n)
        g[o:o + n] = (k.astype(np.float64) / alpha).astype(F)  # exact: alpha is a power of two
        o, n = offs[WILD_T], numels[WILD_T]
        g[o + 5] = F((q + 0.5) / alpha)
        g[o + 6] = F(-(q + 7.25) / alpha)
        g[o + 7] = F(np.nan)
        g[o + 8] = F(np.inf)
        g[o + 9] = F(-np.inf)
        g[o + 8190] = F(1e30)
    return g


def mix32(x):
    x = np.asarray(x, dtype=np.uint64) & M32
    x ^= x >> np.uint64(16)
    x = (x * np.uint64(0x7FEB352D)) & M32
    x ^= x >> np.uint64(15)
    x = (x * np.uint64(0x846CA68B)) & M32
    x ^= x >> np.uint64(16)
    return x


def stream_key(seed, step, rank):
    k = int(mix32((step * 0x9E3779B9 + rank * 0x85EBCA6B + 0x632BE59B) & M32))
    return int(mix32((seed & M32) ^ k))


def uniform(idx, key):
    """24 random bits of mix32(idx ^ key) as fp32 in [0, 1)."""
    h = mix32((np.asarray(idx, dtype=np.uint64) & M32) ^ np.uint64(key & M32))
    return (h >> np.uint64(8)).astype(F) * F(1.0 / 16777216.0)


def chunk_rows(offs, numels):
    """(start, length) of every chunk row: each tensor cut into rows of 8192 elements."""
    rows = []
    for o, n in zip(offs, numels):
        for j in range(0, n, CHUNK):
            rows.append((o + j, min(CHUNK, n - j)))
    return rows


def encode(g, offs, numels, bucket_offset, alpha, inv_a, q, key, resid=None):
    """-> (int8 codes [L], per-row saturation counts); ``resid`` (fp32 [L]) updated in place."""
    L = g.shape[0]
    codes = np.zeros(L, dtype=np.int8)
    sat = []
    alpha, inv_a = F(alpha), F(inv_a)
    with np.errstate(all="ignore"):
        for start, ln in chunk_rows(offs, numels):
            sl = slice(start, start + ln)
            acc = g[sl].astype(F)
            if resid is not None:
                acc = (acc + resid[sl]).astype(F)
            y = (acc * alpha).astype(F)
            f = np.floor(y)
            u = uniform(bucket_offset + start + np.arange(ln), key)
            frac = (y - f).astype(F)
            up = np.zeros(ln, dtype=F)
            up[u < frac] = 1.0  # a NaN fraction (y infinite or NaN) compares false
            c = (f + up).astype(F)
            nan = np.isnan(y)
            c = np.where(nan, F(0), np.minimum(np.maximum(c, F(-q)), F(q)))
            ci = c.astype(np.int32)
            codes[sl] = ci.astype(np.int8)
            sat.append(int(np.count_nonzero(nan | (y < -q) | (y > q))))
            if resid is not None:
                resid[sl] = (acc - (ci.astype(F) * inv_a).astype(F)).astype(F)
    return codes, np.array(sat, dtype=np.int32)


def row_sumsq(d):
    """One chunk row's fp32 sum of d * d (len <= 8192) in the kernels' order: thread t of 256 adds,
    from 0, the elements u * 1024 + 4 t + j for u = 0..7 outer and j = 0..3 inner; per wave of 64
    the shuffle-down tree; then the four waves in order."""
    x = np.zeros(CHUNK, dtype=F)
    x[:d.shape[0]] = d
    with np.errstate(all="ignore"):
        sq = (x * x).astype(F).reshape(8, 256, 4)
        s = np.zeros(256, dtype=F)
        for u in range(8):
            for j in range(4):
                s = (s + sq[u, :, j]).astype(F)
        w = s.reshape(4, 64)
        k = 32
        while k:
            w = (w[:, :k] + w[:, k:2 * k]).astype(F)
            k >>= 1
        t = w[0, 0]
        for i in range(1, 4):
            t = F(t + w[i, 0])
    return t


def update_partials(p_new, p_old, offs, numels):
    with np.errstate(all="ignore"):
        d = (p_new - p_old).astype(F)
    return np.array([row_sumsq(d[s:s + n]) for s, n in chunk_rows(offs, numels)], dtype=F)


def alpha_rule(partials, r, steps, lr, numel, world):
    """-> (r, alpha, inv_a, inv_na): fp64 throughout, the three scales rounded to fp32."""
    s = 0.0
    for v in partials:
        s += float(v)
    r = BETA * r + (1.0 - BETA) * s if steps else s
    den = 2.0 * world * r + EPS2
    with np.errstate(all="ignore"):
        a64 = float(F(lr)) * math.sqrt(numel) / math.sqrt(den) if den >= 0 else float("nan")
        alpha = F(a64)
        if alpha == 0:
            return r, alpha, F(0), F(0)
        return (r, alpha, F(np.float64(1.0) / np.float64(alpha)),
                F(np.float64(1.0) / (np.float64(alpha) * np.float64(world))))


def sgd(p, m, g, lr, momentum, wd, nesterov, first):
    """SGD with dampening 0 in fp32, every product and sum rounded on its own, in place."""
    lr, mu, wd = F(lr), F(momentum), F(wd)
    with np.errstate(all="ignore"):
        d = g.astype(F)
        if wd != 0:
            d = (d + (wd * p).astype(F)).astype(F)
        if mu != 0:
            m[:] = d if first else ((m * mu).astype(F) + d).astype(F)
            d = (d + (mu * m).astype(F)).astype(F) if nesterov else m.copy()
        p[:] = (p - (lr * d).astype(F)).astype(F)


def apply(summed, p, m, offs, numels, inv_na, lr, momentum, wd=0.0, nesterov=False, first=False):
    """The receive side on one bucket: int8 sums -> g^ -> SGD on the tensors' own elements;
    returns the rows' update partials."""
    old = p.copy()
    with np.errstate(all="ignore"):
        g = (summed.astype(np.int8).astype(F) * F(inv_na)).astype(F)
    for o, n in zip(offs, numels):
        sl = slice(o, o + n)
        pv, mv = p[sl], m[sl]
        sgd(pv, mv, g[sl], lr, momentum, wd, nesterov, first)
    return update_partials(p, old, offs, numels)


class Training:
    """N ranks training one flat model of several buckets on prescribed gradients: the dense first
    step, then the int8 exchange.  ``buckets``: list of (numels, offsets, length); bucket b starts
    at the sum of the lengths before it."""

    def __init__(self, buckets, world, p0, lr, momentum, seed, ef=False):
        self.buckets, self.N, self.q = buckets, world, q_of(world)
        self.lr, self.mu, self.seed = lr, momentum, seed
        self.starts = np.cumsum([0] + [b[2] for b in buckets])[:-1].tolist()
        self.numel = sum(sum(b[0]) for b in buckets)
        self.p = p0.astype(F).copy()
        self.m = np.zeros_like(self.p)
        self.resid = [np.zeros_like(self.p) for _ in range(world)] if ef else None
        self.r, self.steps, self.opt_steps, self.step_idx = 0.0, 0, 0, 0
        self.alpha = self.inv_a = self.inv_na = F(0)
        self.sat = [0] * world

    def _scale(self, partials):
        self.r, self.alpha, self.inv_a, self.inv_na = alpha_rule(
            partials, self.r, self.steps, self.lr, self.numel, self.N)
        self.steps += 1

    def step(self, grads):
        """``grads``: one fp32 [total] array per rank."""
        first = self.opt_steps == 0
        partials = []
        if self.steps == 0:  # dense: the fp32 sum (exact for the tests' dyadic gradients) / N
            tot = np.zeros_like(self.p)
            for g in grads:
                tot = (tot + g).astype(F)
            g = (tot * F(1.0 / self.N)).astype(F)
            old = self.p.copy()
            for (numels, offs, ln), s0 in zip(self.buckets, self.starts):
                sl = slice(s0, s0 + ln)  # the optimizer steps the whole range, pads included
                pv, mv = self.p[sl], self.m[sl]
                sgd(pv, mv, g[sl], self.lr, self.mu, 0.0, False, first)
            for (numels, offs, ln), s0 in zip(self.buckets, self.starts):
                partials += list(update_partials(self.p[s0:s0 + ln], old[s0:s0 + ln], offs,
                                                 numels))
        else:
            self.sat = [0] * self.N
            for (numels, offs, ln), s0 in zip(self.buckets, self.starts):
                sl = slice(s0, s0 + ln)
                tot = np.zeros(ln, dtype=np.int32)
                for rk, g in enumerate(grads):
                    key = stream_key(self.seed, self.step_idx, rk)
                    rs = None if self.resid is None else self.resid[rk][sl]
                    c, st = encode(g[sl], offs, numels, s0, self.alpha, self.inv_a, self.q, key, rs)
                    tot += c
                    self.sat[rk] += int(st.sum())
                assert np.abs(tot).max() <= 127
                pv, mv = self.p[sl], self.m[sl]
                partials += list(apply(tot.astype(np.int8), pv, mv, offs, numels, self.inv_na,
                                       self.lr, self.mu, first=first))
        self._scale(partials)
        self.opt_steps += 1
        self.step_idx += 1


# ---- the real exchange, driven with prescribed gradients ---------------------------------------
SHAPES = [(40, 50), (10,), (3 * CHUNK + 17,), (7,), (64,)]
BUCKET_BYTES = 16 << 10  # two buckets: [2000, 10] | [24593, 7, 64]
LR, MOMENTUM, EX_SEED = 2.0 ** -4, 0.9, 3  # lr a power of two: lr * d is exact, fused or not


def grad_of(step, rank, n):
    """Dyadic gradients (multiples of 2^-12 below 1/8): their fp32 sum over the ranks is exact,
    so the dense first step does not depend on the order of the all-reduce."""
    rs = np.random.RandomState(1000 * step + rank + 1)
    return (rs.randint(-512, 513, size=n).astype(np.float64) / 4096.0).astype(F)


def make_flat(device="cpu"):
    import torch
    from ewdml.parallel.flat import FlatModel

    gen = torch.Generator().manual_seed(7)
    params = [torch.nn.Parameter((torch.randn(*s, generator=gen) * 0.1).to(device))
              for s in SHAPES]
    return FlatModel(params, bucket_bytes=BUCKET_BYTES, reverse=False)


def same_bits(a, b):
    import torch

    a = torch.as_tensor(a).detach().cpu().contiguous()
    b = torch.as_tensor(b).detach().cpu().contiguous()
    return a.shape == b.shape and torch.equal(a.view(torch.int32), b.view(torch.int32))


def run_rank(rank, world, steps, ef=False, device="cpu"):
    import torch
    from ewdml.compress import make_codec
    from ewdml.optim.flat import FlatSGD
    from ewdml.parallel.comm import Comm
    from ewdml.parallel.intsgd import IntSGDExchange

    flat = make_flat(device)
    opt = FlatSGD(flat, lr=LR, momentum=MOMENTUM, weight_decay=0.0)
    ex = IntSGDExchange(flat, Comm(), make_codec("intsgd", seed=EX_SEED), opt, error_feedback=ef)
    alphas, stats = [], []
    for step in range(steps):
        flat.grad.copy_(torch.from_numpy(grad_of(step, rank, flat.numel)).to(device))
        ex.begin()
        ex.finish()
        st = ex.last
        stats.append((st.payload_bytes, st.wire_bytes_sent, st.wire_bytes_recv, st.collectives))
        alphas.append(ex.codec.int_state.values()["alpha"])
    return {"params": flat.data.clone().cpu(), "mom": opt.mom.clone().cpu(),
            "resid": None if ex.resid is None else ex.resid.clone().cpu(),
            "alphas": alphas, "stats": stats, "state": ex.state(), "health": ex.codec_health(),
            "lengths": [b.length for b in flat.buckets], "numel": flat.numel,
            "buckets": len(flat.buckets)}


def simulate(world, steps, ef=False):
    """All ``world`` ranks in numpy: the common parameters / momentum, every rank's residual and
    the scale after every step."""
    flat = make_flat()
    buckets = [(list(b.plan.numels), list(b.plan.offsets), b.length) for b in flat.buckets]
    assert [b.start for b in flat.buckets] == np.cumsum([0] + [b[2] for b in buckets])[:-1].tolist()
    tr = Training(buckets, world, flat.data.detach().numpy(), LR, MOMENTUM, EX_SEED, ef)
    alphas = []
    for step in range(steps):
        tr.step([grad_of(step, r, flat.numel) for r in range(world)])
        alphas.append(float(tr.alpha))
    return {"params": tr.p, "mom": tr.m, "resid": tr.resid, "alphas": alphas, "r": tr.r}
