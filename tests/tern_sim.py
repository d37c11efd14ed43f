"""A second opinion for the TernGrad oracle (compress/oracle.py encode_tern): the same codec written
again in plain numpy and Python loops -- its own counter RNG, its own summation order, its own
layout arithmetic and its own bit packing -- sharing no code with the oracle.  Also the fixed
bucket of edge-case tensors that the codec's CPU and GPU tests share."""
import numpy as np

F = np.float32
CHUNK = 8192
M32 = 0xFFFFFFFF

# the one-element tensor, the 16-code pad on both sides, the chunk edge on both sides, and a
# three-chunk tensor (the cross-chunk sum order)
NUMELS = [1, 15, 16, 17, 1000, 8191, 8192, 8193, 20000]
# tensors overwritten by bucket(): all zeros | constant | one outlier
ZERO_T, CONST_T, OUTLIER_T = 3, 2, 4
OUTLIER = 100.0
BUCKET_OFFSET = 4096


def offsets(numels=NUMELS):
    """Tensors packed at multiples of 64 elements (parallel/flat.py): (offsets, bucket length)."""
    offs, o = [], 0
    for n in numels:
        offs.append(o)
        o += (n + 63) // 64 * 64
    return offs, o


def bucket(seed=0, numels=NUMELS):
    """fp32 bucket of fixed-seed normal draws (0 between the tensors) with one all-zero tensor, one
    constant tensor and one tensor of N(0, 1) values holding a single outlier of 100."""
    offs, length = offsets(numels)
    rs = np.random.RandomState(1234 + seed)
    g = np.zeros(length, dtype=F)
    for t, (o, n) in enumerate(zip(offs, numels)):
        g[o:o + n] = (rs.standard_normal(n) * (0.02 * (t + 1))).astype(F)
    if numels is NUMELS:
        o, n = offs[ZERO_T], numels[ZERO_T]
        g[o:o + n] = 0.0
        o, n = offs[CONST_T], numels[CONST_T]
        g[o:o + n] = F(-0.375 if seed % 2 else 0.375)
        o, n = offs[OUTLIER_T], numels[OUTLIER_T]
        g[o:o + n] = rs.standard_normal(n).astype(F)
        g[o + 123] = F(OUTLIER if seed % 2 == 0 else -OUTLIER)
    return g


def mix32(x):
    x = int(x) & M32
    x ^= x >> 16
    x = (x * 0x7FEB352D) & M32
    x ^= x >> 15
    x = (x * 0x846CA68B) & M32
    x ^= x >> 16
    return x


def stream_key(seed, step, rank):
    k = mix32((step * 0x9E3779B9 + rank * 0x85EBCA6B + 0x632BE59B) & M32)
    return mix32((seed & M32) ^ k)


def uniform(idx, key):
    """24 random bits of mix32(idx ^ key) as an fp32 in [0, 1)."""
    return F(mix32((int(idx) & M32) ^ (key & M32)) >> 8) * F(1.0 / 16777216.0)


def _tree256(s):
    """256 per-thread fp32 values -> one: per wave of 64 the shuffle-down tree, then waves 0..3."""
    tot = F(0.0)
    for w in range(4):
        x = list(s[64 * w:64 * w + 64])
        d = 32
        while d:
            for lane in range(d):
                x[lane] = F(x[lane] + x[lane + d])
            d >>= 1
        tot = F(tot + x[0])
    return tot


def sumsq(x):
    """fp32 sum of x * x in the kernels' order.  Per 8192-chunk thread t of 256 adds the elements u
    * 1024 + 4 t + j (u outer, j inner; absent ones add +0), then the tree; across chunks thread t
    adds the chunk sums t, t + 256, ..., then the tree again."""
    x = np.asarray(x, dtype=F)
    parts = []
    for c0 in range(0, len(x), CHUNK):
        row = np.zeros(CHUNK, dtype=F)
        seg = x[c0:c0 + CHUNK]
        row[:len(seg)] = seg * seg
        s = [F(0.0)] * 256
        for t in range(256):
            a = F(0.0)
            for u in range(CHUNK // 1024):
                for j in range(4):
                    a = F(a + row[u * 1024 + 4 * t + j])
            s[t] = a
        parts.append(_tree256(s))
    s = [F(0.0)] * 256
    for k, p in enumerate(parts):
        s[k % 256] = F(s[k % 256] + p)
    return _tree256(s)


def scale_of(x, clip):
    """min(max|x|, clip * sqrt(sumsq / n)) in fp32, one rounding per operation; clip 0: max|x|."""
    x = np.asarray(x, dtype=F)
    absmax = F(np.max(np.abs(x)))
    if not clip > 0:
        return absmax
    rms = F(np.sqrt(F(sumsq(x) / F(len(x)))))
    return min(absmax, F(F(clip) * rms))


def layout(numels):
    """(byte offset of the codes, code word of every tensor's first element, payload bytes)."""
    T = len(numels)
    codes = (4 * T + 15) // 16 * 16
    word0, w = [], 0
    for n in numels:
        word0.append(w)
        w += (n + 15) // 16
    return codes, word0, (codes + 4 * w + 15) // 16 * 16


def encode(g, numels, offs, bucket_offset, clip, key, residual=None):
    """-> (payload uint8, the scalers, the new residual or None).  ``g`` and ``residual`` are the
    bucket's fp32 arrays; neither is modified."""
    g = np.asarray(g, dtype=F)
    x_all = g if residual is None else (g + np.asarray(residual, dtype=F)).astype(F)
    codes_at, word0, nbytes = layout(numels)
    pay = np.zeros(nbytes, dtype=np.uint8)
    words = np.zeros((nbytes - codes_at) // 4, dtype=np.uint32)
    scales = np.zeros(len(numels), dtype=F)
    new_res = None if residual is None else x_all.copy()
    for t, (o, n) in enumerate(zip(offs, numels)):
        x = x_all[o:o + n]
        sc = F(scale_of(x, clip))
        scales[t] = sc
        inv = F(1.0) / sc if sc > 0 else F(0.0)
        for i in range(n):
            lvl = F(abs(x[i]) * inv)
            fl = F(np.floor(lvl))
            up = uniform(bucket_offset + o + i, key) < F(lvl - fl)
            q = min(F(fl + (F(1.0) if up else F(0.0))), F(1.0))
            code = 0 if q == 0 else (3 if x[i] < 0 else 1)
            words[word0[t] + i // 16] |= np.uint32(code << (2 * (i % 16)))
            if new_res is not None:
                dec = F(0.0) if code == 0 else (F(-sc) if code == 3 else sc)
                new_res[o + i] = F(x[i] - dec)
    pay[:4 * len(numels)] = scales.view(np.uint8)
    pay[codes_at:codes_at + 4 * len(words)] = words.view(np.uint8)
    return pay, scales, new_res


def decode(pay, numels, offs, length):
    """One payload decoded: fp32 [length], 0 between the tensors."""
    pay = np.asarray(pay, dtype=np.uint8)
    codes_at, word0, nbytes = layout(numels)
    scales = pay[:4 * len(numels)].view(F)
    words = pay[codes_at:nbytes].view(np.uint32)
    out = np.zeros(length, dtype=F)
    for t, (o, n) in enumerate(zip(offs, numels)):
        for i in range(n):
            code = (int(words[word0[t] + i // 16]) >> (2 * (i % 16))) & 3
            assert code != 2, "the code 2 is never written"
            out[o + i] = F(0.0) if code == 0 else (F(-scales[t]) if code == 3 else scales[t])
    return out


def decode_mean(pays, numels, offs, length, scale):
    """scale * (rank-ordered fp32 sum from 0 of the decoded payloads)."""
    acc = np.zeros(length, dtype=F)
    for p in pays:
        acc = (acc + decode(p, numels, offs, length)).astype(F)
    return (acc * F(scale)).astype(F)
