"""Shared by the 8-bit Adam tests: shapes, inputs and a float64 reference of the format and the step
that shares no code with ``compress/oracle.py``.  Map entries and midpoints are rounded to fp32
(the stored format) and used as float64; absmax stays float64.  ``near`` marks elements whose ``x``
lies within relative 2^-18 of a midpoint, where an fp32 implementation may land one code off."""
import numpy as np
import torch

from tests import optim_ref as R

BLOCK, SLOTS, CHUNK, ZERO = 256, 32, 8192, 127
# tensor sizes of a range: one short block; a full block and a short one; a chunk boundary then a
# short chunk; and the three together (64-aligned offsets, a pad after every tensor)
RANGES = {"64": [64], "320": [320], "8512": [8192 + 320], "all": [64, 320, 8192 + 320]}
HP = dict(lr=1e-3, beta1=0.9, beta2=0.999, eps=1e-8)


def books():
    """(map_m, mid_m, map_v, mid_v): decade i = 0..6 holds n_i (2^i signed, 2^(i+1) unsigned)
    equal bins on [0.1, 1], each bin's mean scaled by 10^(i-6); plus 0 and 1."""
    out = []
    for signed in (True, False):
        vals = [0.0, 1.0]
        for i in range(7):
            n = 2 ** i if signed else 2 ** (i + 1)
            e = 0.1 + 0.9 * np.arange(n + 1) / n
            means = (e[:-1] + e[1:]) / 2.0 * 10.0 ** (i - 6)
            vals += list(means) + (list(-means) if signed else [])
        m = np.sort(np.array(vals)).astype(np.float32).astype(np.float64)
        mid = ((m[:-1] + m[1:]) / 2.0).astype(np.float32).astype(np.float64)
        out += [torch.from_numpy(m), torch.from_numpy(mid)]
    return out


def layout(numels):
    """(length, blocks, chunks, pad mask); blocks = one (offset, numel, absmax slot0) per tensor."""
    blocks, o, c = [], 0, 0
    for n in numels:
        blocks.append((o, n, SLOTS * c))
        o += (n + 63) // 64 * 64 + 64
        c += (n + CHUNK - 1) // CHUNK
    pad = torch.ones(o, dtype=torch.bool)
    for off, n, _ in blocks:
        pad[off:off + n] = False
    return o, blocks, c, pad


def inputs(name, steps, gdt=torch.float32):
    """``(p0, [g_1 .. g_steps])``.  Every tensor's first element carries its block's largest
    gradient, negative.  Where the last tensor has a second block, its first is zero in ``p0``
    and every gradient and its second has one gradient 10^4 times the rest.  Pads hold values."""
    length, blocks, _, _ = layout(RANGES[name])
    gen = torch.Generator().manual_seed(1000 + sum(RANGES[name]))
    p0 = torch.randn(length, generator=gen) * 1e-2
    o, n, _ = blocks[-1]
    grads = []
    for s in range(steps):
        g = torch.randn(length, generator=gen) * (0.5 + float(torch.rand(1, generator=gen)))
        for off, _, _ in blocks:
            g[off] = -6.0 - s
        if n > BLOCK + 8:
            g[o:o + BLOCK] = 0.0
            g[o + BLOCK:o + min(n, 2 * BLOCK)] *= 1e-3
            g[o + BLOCK + 5] = 10.0
            if n > 2 * BLOCK:
                g[o + 2 * BLOCK] = -6.0 - s
        grads.append(g.to(gdt))
    if n > BLOCK + 8:
        p0[o:o + BLOCK] = 0.0
    return p0, grads


def quantize64(val, amax, mid, zero):
    """Codes ``#{k : mid[k] < val / amax}`` of [blocks, 256] values (absmax 0: ``zero``), and near."""
    dead = (amax == 0)[:, None].expand_as(val)
    x = val / torch.where(amax == 0, torch.ones_like(amax), amax)[:, None]
    code = torch.bucketize(x, mid)
    near = torch.zeros_like(dead)
    for k in (code - 1, code):
        b = mid[k.clamp(0, mid.numel() - 1)]
        near |= (x - b).abs() <= 2.0 ** -18 * b.abs()
    return torch.where(dead, torch.full_like(code, zero), code), near & ~dead


def fresh(length, chunks):
    return [torch.full((length,), ZERO), torch.zeros(length, dtype=torch.int64),
            torch.zeros(SLOTS * chunks, dtype=torch.float64),
            torch.zeros(SLOTS * chunks, dtype=torch.float64)]


def step64(p, cm, cv, am, av, g, blocks, t, **hp):
    """Step ``t`` (1-based) in place: ``optim_ref.adam64`` on the dequantised moments, then the
    requantise (a ``v > 0`` takes code 1 at least).  Returns ``(near_m, near_v)`` over the range."""
    map_m, mid_m, map_v, mid_v = books()
    near = torch.zeros(2, p.numel(), dtype=torch.bool)
    for off, n, s0 in blocks:
        nb = (n + BLOCK - 1) // BLOCK
        sl, sb = slice(off, off + n), slice(s0, s0 + nb)
        m = map_m[cm[sl]] * torch.repeat_interleave(am[sb], BLOCK)[:n]
        v = map_v[cv[sl]] * torch.repeat_interleave(av[sb], BLOCK)[:n]
        pt = p[sl].clone()
        R.adam64(pt, m, v, None, g[sl], t, **hp)
        p[sl] = pt
        m, v = (torch.nn.functional.pad(a, (0, nb * BLOCK - n)).view(nb, BLOCK) for a in (m, v))
        am[sb], av[sb] = m.abs().amax(dim=1), v.amax(dim=1)
        qm, nm = quantize64(m, am[sb], mid_m, ZERO)
        qv, nv = quantize64(v, av[sb], mid_v, 0)
        qv = torch.where((v > 0) & (qv == 0), torch.ones_like(qv), qv)
        cm[sl], cv[sl] = qm.view(-1)[:n], qv.view(-1)[:n]
        near[0, sl], near[1, sl] = nm.view(-1)[:n], nv.view(-1)[:n]
    return near
