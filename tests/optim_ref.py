"""Shared by the SGD / Adam tests: an independent reference of both rules (it shares no code with
``compress/oracle.py``), twice.

``sgd64`` / ``adam64``: float64 throughout.  The hyper-parameters (lr, momentum, dampening, weight
decay, the betas, eps) and ``grad_scale`` are first rounded to fp32 and ``g * grad_scale`` is
rounded to fp32 before use: these are the values the kernels receive.  Adam's bias correction
``lr_step = lr * sqrt(1 - b2^t) / (1 - b1^t)`` uses the same fp32-rounded betas, which is what the
kernel's device-step path computes (``ew_adam_resolve``).  ``FlatAdam``'s host formula uses the
double betas and so differs from this by about 6.7e-6 relative in ``lr_step`` (0.9 and 0.999 move
by 2.4e-8 and 1.3e-8 when rounded, and ``1 - b^t`` is small at small t); that is by design and is
not to be "fixed": on the GPU the host value is never used.  ``round_hp=False`` switches every
rounding off (the comparison with ``torch.optim`` in float64).

``sgd32`` / ``adam32``: fp32 torch on the CPU, every product and sum its own op and so rounded on
its own, in the evaluation order of ``ew_sgd`` / ``ew_adam`` (``ops/csrc/common.h``, ``optim.hip``),
``1 - dampening`` and ``1 - beta`` formed in fp32, the square root correctly rounded (``sqrt32``:
torch's own on the CPU is not).  The extension is built with
``-ffp-contract=off``, so this is the kernels' bitwise definition.

Adam in the project's reference form: ``denom = sqrt(v) + eps`` (not ``sqrt(v / bc2) + eps``).
All four step functions work in place on 1-D tensors and take the raw gradient (fp32, bf16 or
fp16)."""
import math

import numpy as np
import torch

F32, F64 = torch.float32, torch.float64


def r32(x, on=True):
    """``x`` rounded to fp32, as a Python float."""
    return float(np.float32(x)) if on else float(x)


def lr_step64(lr, beta1, beta2, t, round_hp=True):
    """Adam's step size at the 1-based step ``t``, in double from the fp32-rounded values."""
    lr, b1, b2 = (r32(x, round_hp) for x in (lr, beta1, beta2))
    return lr * math.sqrt(1.0 - b2 ** t) / (1.0 - b1 ** t)


def _grad64(g, grad_scale, round_hp):
    g = g.to(F64) * r32(grad_scale, round_hp)  # exact in double: one rounding below
    return g.to(F32).to(F64) if round_hp else g


def _grad32(g, grad_scale):
    return g.to(F32) * torch.tensor(grad_scale, dtype=F32)


def sgd64(p, buf, g, *, lr, momentum=0.0, dampening=0.0, weight_decay=0.0, nesterov=False,
          first=False, grad_scale=1.0, round_hp=True):
    assert p.dtype == F64 and buf.dtype == F64
    lr, mu, damp, wd = (r32(x, round_hp) for x in (lr, momentum, dampening, weight_decay))
    d = _grad64(g, grad_scale, round_hp)
    if wd != 0.0:
        d = d + wd * p
    if mu != 0.0:
        buf.copy_(d if first else buf * mu + (1.0 - damp) * d)
        d = d + mu * buf if nesterov else buf
    p.copy_(p - lr * d)


def sgd32(p, buf, g, *, lr, momentum=0.0, dampening=0.0, weight_decay=0.0, nesterov=False,
          first=False, grad_scale=1.0):
    assert p.dtype == F32 and buf.dtype == F32
    lr, mu, damp, wd = (torch.tensor(x, dtype=F32) for x in (lr, momentum, dampening,
                                                            weight_decay))
    one = torch.tensor(1.0, dtype=F32)
    d = _grad32(g, grad_scale)
    if float(wd) != 0.0:
        d = d + wd * p
    if float(mu) != 0.0:
        buf.copy_(d if first else buf * mu + (one - damp) * d)
        d = d + mu * buf if nesterov else buf
    p.copy_(p - lr * d)


def adam64(p, m, v, vmax, g, t, *, lr, beta1, beta2, eps, weight_decay=0.0, amsgrad=False,
           grad_scale=1.0, round_hp=True):
    """Step ``t`` (1-based).  ``vmax`` is only touched by AMSGrad (None otherwise is fine)."""
    assert all(x.dtype == F64 for x in (p, m, v))
    step = lr_step64(lr, beta1, beta2, t, round_hp)
    b1, b2, eps, wd = (r32(x, round_hp) for x in (beta1, beta2, eps, weight_decay))
    g = _grad64(g, grad_scale, round_hp)
    if wd != 0.0:
        g = g + wd * p
    m.copy_(m * b1 + (1.0 - b1) * g)
    v.copy_(v * b2 + (1.0 - b2) * (g * g))
    if amsgrad:
        vmax.copy_(torch.maximum(vmax, v))
        d = vmax.sqrt() + eps
    else:
        d = v.sqrt() + eps
    p.copy_(p - step * (m / d))


def sqrt32(x):
    """Correctly rounded fp32 square root.  ``torch.sqrt`` on the CPU is not (a vector math
    library within 1 ulp: about one value in a thousand is off by one); numpy's is the
    processor's IEEE instruction, like the kernels' ``sqrtf``."""
    assert x.dtype == F32
    return torch.from_numpy(np.sqrt(x.contiguous().numpy()))


def adam32(p, m, v, vmax, g, lr_step, *, beta1, beta2, eps, weight_decay=0.0, amsgrad=False,
           grad_scale=1.0):
    """One step with the step size ``lr_step`` as the kernel receives it (rounded to fp32 here)."""
    assert all(x.dtype == F32 for x in (p, m, v))
    step, b1, b2, eps, wd = (torch.tensor(x, dtype=F32) for x in (lr_step, beta1, beta2, eps,
                                                                  weight_decay))
    one = torch.tensor(1.0, dtype=F32)
    g = _grad32(g, grad_scale)
    if float(wd) != 0.0:
        g = g + wd * p
    m.copy_(m * b1 + (one - b1) * g)
    v.copy_(v * b2 + (one - b2) * (g * g))
    if amsgrad:
        vmax.copy_(torch.maximum(vmax, v))
        d = sqrt32(vmax) + eps
    else:
        d = sqrt32(v) + eps
    p.copy_(p - step * (m / d))


# ---- the bound against float64 -------------------------------------------------------------------
def err(x, x64):
    return float((x.to(F64) - x64).abs().max())


def limit(x32, x64):
    """How far a correct fp32 implementation may be from ``x64``: four times what the fp32
    reference (``x32``, computed on the CPU, never by the code under test) is, and no less than
    one ulp of the largest value.  The factor 4 covers a device ``lr_step`` one fp32 ulp away from
    the host's (``pow`` in double is not correctly rounded) and a one-ulp difference in ``sqrt`` or
    the divide."""
    return max(4.0 * err(x32, x64), 2.0 ** -23 * float(x64.abs().max()))


def check(name, got, x32, x64, tag=""):
    """Print and assert ``err(got) <= limit``; returns (err, limit)."""
    e, lim = err(got, x64), limit(x32, x64)
    print(f"{tag}{name}: err {e:.3e} limit {lim:.3e} (ref32 err {err(x32, x64):.3e})")
    assert e <= lim, f"{tag}{name}: |x - x64| max {e:.3e} > {lim:.3e}"
    return e, lim
