"""Shared by the LARS / LAMB tests: the flat test model and an independent per-tensor float64
implementation of both rules (``FlatLARS`` / ``FlatLAMB`` are checked against it; it shares no
code with ``compress/oracle.py``)."""
import math

import torch

from ewdml.parallel.flat import FlatModel

# a 1-D tensor (never adapts), a small matrix, exactly one chunk, one chunk + 1 (scalar tail), five
# rows of 4000 (three chunks, the last partial)
SHAPES = [(10,), (3, 7), (64, 128), (1, 8193), (5, 4000)]


def make_flat(shapes=SHAPES, seed=0, device="cpu", bucket_bytes=8 << 20):
    """A FlatModel over parameters of ``shapes`` (flat order = list order)."""
    gen = torch.Generator().manual_seed(seed)
    ps = [torch.nn.Parameter((torch.randn(s, generator=gen)
                              * (0.05 + float(torch.rand(1, generator=gen)))).to(device))
          for s in shapes]  # Parameter(...) of the moved tensor: a leaf on ``device``
    return FlatModel(ps, bucket_bytes=bucket_bytes, reverse=False)


def make_grad(flat, seed, dtype=torch.float32):
    """A flat gradient with zero padding, its values exactly representable in ``dtype``."""
    gen = torch.Generator().manual_seed(1000 + seed)
    g = torch.zeros(flat.numel)
    for o, p in zip(flat.offsets, flat.params):
        n = p.numel()
        g[o:o + n] = torch.randn(n, generator=gen) * (0.01 + float(torch.rand(1, generator=gen)))
    return g.to(dtype).to(flat.data.device)


def split(flat, vec):
    """Per-tensor float64 copies of a flat vector."""
    return [vec[o:o + p.numel()].detach().double().cpu() for o, p in zip(flat.offsets, flat.params)]


class Ref64:
    """LARS / LAMB per tensor in float64.  ``p`` / ``s1`` / ``s2``: lists of float64 tensors
    (parameters; LARS momentum buffer or LAMB exp_avg; LAMB exp_avg_sq)."""

    def __init__(self, kind, flat, lr, weight_decay=0.0, eta=0.001, momentum=0.0, dampening=0.0,
                 nesterov=False, betas=(0.9, 0.999), eps=1e-8):
        self.kind, self.lr, self.wd, self.eta = kind, lr, weight_decay, eta
        self.momentum, self.dampening, self.nesterov = momentum, dampening, nesterov
        self.betas, self.eps = betas, eps
        self.p = split(flat, flat.data)
        self.s1 = [torch.zeros_like(x) for x in self.p]
        self.s2 = [torch.zeros_like(x) for x in self.p]
        self.adapts = [q.dim() >= 2 for q in flat.params]
        self.t = 0
        self.ratios = [1.0] * len(self.p)

    def step(self, grads, grad_scale=1.0):
        """``grads``: per-tensor float64 raw gradients."""
        self.t += 1
        for i, (p, raw) in enumerate(zip(self.p, grads)):
            g = raw * grad_scale
            pn = math.sqrt(float((p * p).sum()))
            if self.kind == "lars":
                gn = math.sqrt(float((g * g).sum()))
                r = 1.0
                if self.adapts[i] and pn > 0 and gn > 0:
                    r = self.eta * pn / (gn + self.wd * pn)
                d = r * (g + self.wd * p)
                if self.momentum != 0:
                    if self.t == 1:
                        self.s1[i] = d.clone()
                    else:
                        self.s1[i] = self.momentum * self.s1[i] + (1 - self.dampening) * d
                    d = d + self.momentum * self.s1[i] if self.nesterov else self.s1[i]
                self.p[i] = p - self.lr * d
            else:
                b1, b2 = self.betas
                self.s1[i] = b1 * self.s1[i] + (1 - b1) * g
                self.s2[i] = b2 * self.s2[i] + (1 - b2) * g * g
                mh = self.s1[i] / (1 - b1 ** self.t)
                vh = self.s2[i] / (1 - b2 ** self.t)
                u = mh / (vh.sqrt() + self.eps) + self.wd * p
                un = math.sqrt(float((u * u).sum()))
                r = pn / un if (self.adapts[i] and pn > 0 and un > 0) else 1.0
                self.p[i] = p - self.lr * r * u
            self.ratios[i] = r


def make_pair(kind, flat, lr, weight_decay=0.0, **kw):
    """(the project's optimizer over ``flat``, the float64 reference from the same start)."""
    from ewdml.optim import FlatLAMB, FlatLARS

    ref = Ref64(kind, flat, lr, weight_decay, **kw)
    if kind == "lars":
        opt = FlatLARS(flat, lr=lr, weight_decay=weight_decay, **kw)
    else:
        opt = FlatLAMB(flat, lr=lr, weight_decay=weight_decay, **kw)
    return opt, ref


def assert_state_close(flat, opt, ref, rtol=1e-5, atol=1e-6):
    names = [("p", flat.data, ref.p)]
    if opt.kind == "lamb":
        names += [("exp_avg", opt.exp_avg, ref.s1), ("exp_avg_sq", opt.exp_avg_sq, ref.s2)]
    elif opt.momentum != 0:
        names.append(("mom", opt.mom, ref.s1))
    for name, vec, want in names:
        for i, (got, w) in enumerate(zip(split(flat, vec), want)):
            torch.testing.assert_close(got, w, rtol=rtol, atol=atol,
                                       msg=lambda m, i=i, name=name: f"{name}[{i}]: {m}")


def padding_is_zero(flat, *vecs):
    mask = torch.ones(flat.numel, dtype=torch.bool)
    for o, p in zip(flat.offsets, flat.params):
        mask[o:o + p.numel()] = False
    return all(bool((v.detach().cpu()[mask] == 0).all()) for v in vecs)
