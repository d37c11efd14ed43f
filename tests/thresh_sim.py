"""A second opinion for the threshold-search sparsifier's oracle (compress/oracle.py encode_thresh):
the same codec written again in plain numpy -- its own capacity rule, its own brute-force
threshold (a histogram of the levels, not a sort), its own layout arithmetic -- sharing no code with
the oracle.  Also the fixed bucket of edge-case tensors that the codec's CPU and GPU tests share."""
import numpy as np

F = np.float32
CHUNK = 8192
LEVELS = 32768

# a three-chunk tensor with a short last chunk (5 elements, capacity 1) | one element | zeros, sent
# whole | a constant (every level ties: nothing is sent) | cubed normals (heavy tails) over two
# chunks | a tensor sent whole | normals with a NaN and an inf
NUMELS = [8192 * 3 + 5, 1, 64, 300, 9000, 40, 5000]
ZERO_T, CONST_T, CUBED_T, WHOLE_T, NONFINITE_T = 2, 3, 4, 5, 6
NAN_AT, INF_AT = 17, 4000
RATIO = 0.01
DENSE_BELOW = 64
BUCKET_OFFSET = 4096


def offsets(numels=NUMELS):
    """Tensors packed at multiples of 64 elements (parallel/flat.py): (offsets, bucket length)."""
    offs, o = [], 0
    for n in numels:
        offs.append(o)
        o += (n + 63) // 64 * 64
    return offs, o


def bucket(seed=0, numels=NUMELS):
    """fp32 bucket of fixed-seed normal draws (0 between the tensors) with the edge-case tensors
    above; every seed gives other values and the same structure."""
    offs, length = offsets(numels)
    rs = np.random.RandomState(4321 + seed)
    g = np.zeros(length, dtype=F)
    for t, (o, n) in enumerate(zip(offs, numels)):
        g[o:o + n] = (rs.standard_normal(n) * (0.02 * (t + 1))).astype(F)
    if numels is NUMELS:
        o, n = offs[ZERO_T], numels[ZERO_T]
        g[o:o + n] = 0.0
        o, n = offs[CONST_T], numels[CONST_T]
        g[o:o + n] = F(-0.375 if seed % 2 else 0.375)
        o, n = offs[CUBED_T], numels[CUBED_T]
        g[o:o + n] = (rs.standard_normal(n) ** 3).astype(F)
        o = offs[NONFINITE_T]
        g[o + NAN_AT] = np.nan
        g[o + INF_AT] = -np.inf if seed % 2 else np.inf
    return g


def chunks(numels, offs):
    """[(tensor, bucket start, length)] of every chunk row, tensors in order."""
    return [(t, o + j, min(CHUNK, n - j)) for t, (o, n) in enumerate(zip(offs, numels))
            for j in range(0, n, CHUNK)]


def caps(numels, offs, ratio=RATIO, dense_below=DENSE_BELOW):
    """Per chunk row: the most entries it sends, and its first slot."""
    cap = []
    for t, _, ln in chunks(numels, offs):
        n = numels[t]
        k = n if n <= dense_below else max(1, int(n * ratio))
        cap.append(ln if k == n else max(1, -(-(k * ln) // n)))
    return cap, [sum(cap[:c]) for c in range(len(cap))]


def levels(x):
    return ((np.asarray(x, dtype=F).view(np.uint32) & np.uint32(0x7FFFFFFF)) >> np.uint32(16)) \
        .astype(np.int64)


def threshold(lev, cap):
    """The smallest J in [0, 32768] with #{lev >= J} <= cap, by trying them all."""
    hist = np.bincount(lev, minlength=LEVELS + 1)
    at_least = np.cumsum(hist[::-1])[::-1]  # at_least[J] = #{lev >= J}; 0 at J = 32768
    return int(np.argmax(at_least <= cap))


def layout(numels, offs, ratio=RATIO, dense_below=DENSE_BELOW):
    """(byte offset of the indices, of the values, payload bytes, slots)."""
    cap, _ = caps(numels, offs, ratio, dense_below)
    C, S = len(cap), sum(cap)
    idx = (2 * C + 15) // 16 * 16
    vals = (idx + 2 * S + 15) // 16 * 16
    return idx, vals, (vals + 4 * S + 15) // 16 * 16, S


def encode(g, numels, offs, residual=None, ratio=RATIO, dense_below=DENSE_BELOW):
    """-> (payload uint8, the thresholds, the new residual or None); no argument is modified."""
    g = np.asarray(g, dtype=F)
    with np.errstate(invalid="ignore"):
        acc = g if residual is None else (g + np.asarray(residual, dtype=F)).astype(F)
    cap, slot0 = caps(numels, offs, ratio, dense_below)
    idx_at, vals_at, nbytes, S = layout(numels, offs, ratio, dense_below)
    rows = chunks(numels, offs)
    counts = np.zeros(len(rows), dtype=np.uint16)
    idx = np.zeros(S, dtype=np.uint16)
    vals = np.zeros(S, dtype=F)
    new_res = None if residual is None else np.asarray(residual, dtype=F).copy()
    js = []
    for c, (_, s0, ln) in enumerate(rows):
        x = acc[s0:s0 + ln]
        lev = levels(x)
        J = threshold(lev, cap[c])
        js.append(J)
        sent = np.flatnonzero(lev >= J)
        assert len(sent) <= cap[c]
        counts[c] = len(sent)
        idx[slot0[c]:slot0[c] + len(sent)] = sent
        vals[slot0[c]:slot0[c] + len(sent)] = x[sent]
        if new_res is not None:
            left = x.copy()
            left[sent] = 0.0
            new_res[s0:s0 + ln] = left
    pay = np.zeros(nbytes, dtype=np.uint8)
    pay[:2 * len(rows)] = counts.view(np.uint8)
    pay[idx_at:idx_at + 2 * S] = idx.view(np.uint8)
    pay[vals_at:vals_at + 4 * S] = vals.view(np.uint8)
    return pay, js, new_res


def decode(pay, numels, offs, length, ratio=RATIO, dense_below=DENSE_BELOW):
    """One payload scattered: fp32 [length], 0 where nothing was sent.  A count above the chunk's
    capacity is cut to it and an index at or past the chunk's length is dropped."""
    pay = np.asarray(pay, dtype=np.uint8)
    cap, slot0 = caps(numels, offs, ratio, dense_below)
    idx_at, vals_at, nbytes, S = layout(numels, offs, ratio, dense_below)
    rows = chunks(numels, offs)
    counts = pay[:2 * len(rows)].view(np.uint16)
    idx = pay[idx_at:idx_at + 2 * S].view(np.uint16)
    vals = pay[vals_at:vals_at + 4 * S].view(F)
    out = np.zeros(length, dtype=F)
    for c, (_, s0, ln) in enumerate(rows):
        for s in range(slot0[c], slot0[c] + min(int(counts[c]), cap[c])):
            if idx[s] < ln:
                out[s0 + int(idx[s])] = vals[s]
    return out


def decode_mean(pays, numels, offs, length, scale, ratio=RATIO, dense_below=DENSE_BELOW):
    """scale * (rank-ordered fp32 sum from 0 of the scattered payloads)."""
    acc = np.zeros(length, dtype=F)
    with np.errstate(invalid="ignore"):
        for p in pays:
            acc = (acc + decode(p, numels, offs, length, ratio, dense_below)).astype(F)
        return (acc * F(scale)).astype(F)
