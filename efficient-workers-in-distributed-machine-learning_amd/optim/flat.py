"""Optimizers over the flat parameter buffer with *explicit* gradients.

Parity: ``optim/sgd.py:11-91`` (SGD whose ``step(grads=...)`` takes the averaged gradient received
from the server; momentum buffer initialised to the first gradient, dampening, Nesterov, weight
decay) and ``optim/adam.py:12-94`` (Adam/AMSGrad with explicit gradients).  The reference loops
over parameter tensors; these run one HIP kernel over a flat range (``ops.sgd_flat`` /
``ops.adam_flat``), and the top-k / QSGD exchanges fuse the SGD update into their decode kernel
(``Codec.decode_apply_sgd``) so the averaged gradient never round-trips through HBM.
"""
import math

import torch

from .. import ops
from ..compress import oracle


class DeviceScalar:
    """An fp32 scalar in device memory that the kernels read at run time (a captured HIP graph
    keeps its kernels' arguments frozen, so a learning-rate schedule is fed through this), updated
    by stream-ordered copies from a ring of pinned host slots (no host synchronisation)."""

    def __init__(self, value: float, device):
        self.t = torch.full((1,), float(value), dtype=torch.float32, device=device)
        self._ring = [(torch.zeros(1, dtype=torch.float32).pin_memory(), None) for _ in range(8)]
        self._slot = 0

    def set(self, value: float):
        host, ev = self._ring[self._slot]
        if ev is not None:
            ev.synchronize()  # the slot's previous copy has been consumed
        host[0] = float(value)
        self.t.copy_(host, non_blocking=True)
        ev = torch.cuda.Event()
        ev.record()
        self._ring[self._slot] = (host, ev)
        self._slot = (self._slot + 1) % len(self._ring)


class _LrMixin:
    """``lr`` as a host value mirrored into ``lr_t`` (device) on the GPU."""

    @property
    def lr(self) -> float:
        return self._lr

    @lr.setter
    def lr(self, value: float):
        self._lr = float(value)
        dev = getattr(self, "_lr_dev", None)
        if dev is not None:
            dev.set(self._lr)

    @property
    def lr_t(self):
        dev = getattr(self, "_lr_dev", None)
        return None if dev is None else dev.t

    def _init_lr(self, lr, device):
        self._lr_dev = DeviceScalar(lr, device) if device.type == "cuda" else None
        self._lr = float(lr)


class FlatSGD(_LrMixin):
    fusable = True

    def __init__(self, flat, lr=0.01, momentum=0.0, dampening=0.0, weight_decay=0.0,
                 nesterov=False):
        if nesterov and (momentum <= 0 or dampening != 0):
            raise ValueError("Nesterov momentum requires a momentum and zero dampening")
        self.flat = flat
        self._init_lr(lr, flat.data.device)
        self.momentum, self.dampening = momentum, dampening
        self.weight_decay, self.nesterov = weight_decay, nesterov
        self.mom = torch.zeros_like(flat.data)
        self.steps = 0

    @property
    def first(self) -> bool:
        return self.steps == 0

    def hparams(self) -> dict:
        return dict(lr=self.lr, momentum=self.momentum, dampening=self.dampening,
                    weight_decay=self.weight_decay, nesterov=self.nesterov, lr_t=self.lr_t)

    def step_range(self, start: int, length: int, grad: torch.Tensor, grad_scale: float = 1.0):
        """Apply SGD to ``flat.data[start:start+length]`` with ``grad`` (same length) * scale."""
        p = self.flat.data[start:start + length]
        m = self.mom[start:start + length]
        if p.is_cuda:
            sh = self.flat.shadow[start:start + length] if self.flat.shadow is not None else None
            ops.sgd_flat(p, m, grad, self.lr, self.momentum, self.dampening, self.weight_decay,
                         grad_scale, self.nesterov, self.first, shadow=sh, lr_tensor=self.lr_t)
            return
        g = grad.to(torch.float32)
        if grad_scale != 1.0:
            g = g * grad_scale
        oracle.sgd_apply(p, m, g, self.lr, self.momentum, self.dampening, self.weight_decay,
                         self.nesterov, self.first)

    def step(self, grad: torch.Tensor = None, grad_scale: float = 1.0):
        """Whole-model step (``grad`` defaults to the flat gradient buffer)."""
        self.step_range(0, self.flat.numel, self.flat.grad if grad is None else grad, grad_scale)
        self.end_step()

    def step_bucket_ptrs(self, b, dp, grads, grad_scale: float = 1.0):
        """SGD of bucket ``b`` from its per-tensor gradients ``grads`` (pointer mode), one
        launch; no :meth:`end_step`."""
        p = self.flat.data_view(b)
        m = self.mom[b.start:b.start + b.length]
        ops.sgd_ptrs(dp, grads, p, m, self.lr, self.momentum, self.dampening, self.weight_decay,
                     grad_scale, self.nesterov, self.first, shadow=self.flat.shadow_view(b),
                     lr_tensor=self.lr_t)

    def end_step(self):
        self.steps += 1

    def state_dict(self):
        hp = {k: v for k, v in self.hparams().items() if k != "lr_t"}
        return {"kind": "sgd", "mom": self.mom, "steps": self.steps, **hp}

    def load_state_dict(self, sd):
        self.mom.copy_(sd["mom"])
        self.steps = int(sd["steps"])
        for k in ("lr", "momentum", "dampening", "weight_decay", "nesterov"):
            if k in sd:
                setattr(self, k, sd[k])


class FlatAdam(_LrMixin):
    fusable = False

    def __init__(self, flat, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0,
                 amsgrad=False):
        self.flat = flat
        self._init_lr(lr, flat.data.device)
        self.betas, self.eps = betas, eps
        self.weight_decay, self.amsgrad = weight_decay, amsgrad
        self.exp_avg = torch.zeros_like(flat.data)
        self.exp_avg_sq = torch.zeros_like(flat.data)
        self.max_exp_avg_sq = torch.zeros_like(flat.data) if amsgrad else None
        self.steps = 0
        # device copy of the step count: the kernel derives the bias correction from it, so a
        # captured HIP graph replays the current step's correction (not the capture step's)
        self.step_t = torch.zeros(1, dtype=torch.int32, device=flat.data.device) \
            if flat.data.is_cuda else None

    def step_range(self, start, length, grad, grad_scale=1.0):
        t = self.steps + 1
        b1, b2 = self.betas
        sl = slice(start, start + length)
        p = self.flat.data[sl]
        vmax = self.max_exp_avg_sq[sl] if self.amsgrad else None
        if p.is_cuda:
            lr_step = self.lr * math.sqrt(1 - b2 ** t) / (1 - b1 ** t)
            sh = self.flat.shadow[sl] if self.flat.shadow is not None else None
            ops.adam_flat(p, self.exp_avg[sl], self.exp_avg_sq[sl], vmax, grad, lr_step, b1, b2,
                          self.eps, self.weight_decay, grad_scale, self.amsgrad, shadow=sh,
                          step=self.step_t, lr=self.lr, lr_tensor=self.lr_t)
            return
        g = grad.to(torch.float32) * grad_scale
        oracle.adam_apply(p, self.exp_avg[sl], self.exp_avg_sq[sl],
                          vmax if vmax is not None else torch.empty(0), g, self.lr, b1, b2,
                          self.eps, self.weight_decay, t, self.amsgrad)

    def step(self, grad=None, grad_scale=1.0):
        self.step_range(0, self.flat.numel, self.flat.grad if grad is None else grad, grad_scale)
        self.end_step()

    def end_step(self):
        self.steps += 1
        if self.step_t is not None:
            self.step_t.add_(1)  # on the stream: captured into the step graph

    def state_dict(self):
        return {"kind": "adam", "exp_avg": self.exp_avg, "exp_avg_sq": self.exp_avg_sq,
                "max_exp_avg_sq": self.max_exp_avg_sq, "steps": self.steps, "lr": self.lr}

    def load_state_dict(self, sd):
        self.exp_avg.copy_(sd["exp_avg"])
        self.exp_avg_sq.copy_(sd["exp_avg_sq"])
        if self.amsgrad and sd.get("max_exp_avg_sq") is not None:
            self.max_exp_avg_sq.copy_(sd["max_exp_avg_sq"])
        self.steps = int(sd["steps"])
        if self.step_t is not None:
            self.step_t.fill_(self.steps)
        self.lr = sd.get("lr", self.lr)


class FlatOnebitAdam(FlatAdam):
    """1-bit Adam (Tang et al., ICML 2021; DeepSpeed ``OnebitAdam``).  Steps 1..``freeze_step`` are
    :class:`FlatAdam` on the dense averaged gradient.  From then on (``frozen``) ``exp_avg_sq`` is
    never written again and the exchange, not :meth:`step_range`, runs the step: every rank
    sign-compresses its error-compensated momentum candidate, and the decode writes the average
    into ``exp_avg`` and applies ``p -= lr_step * exp_avg / (sqrt(exp_avg_sq) + eps)``
    (``Codec.encode_momentum`` / ``decode_apply_onebit``).  The error-feedback residual is per-rank
    state and lives in the exchange; this optimizer's state is the same on every rank."""
    onebit = True

    def __init__(self, flat, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0,
                 amsgrad=False, freeze_step=None):
        if amsgrad:
            raise ValueError("1-bit Adam freezes exp_avg_sq: AMSGrad's running maximum has no "
                             "place in it")
        if freeze_step is None or int(freeze_step) < 1:
            raise ValueError("1-bit Adam needs freeze_step >= 1 (the dense warm-up's length)")
        super().__init__(flat, lr=lr, betas=betas, eps=eps, weight_decay=weight_decay)
        self.freeze_step = int(freeze_step)

    @property
    def frozen(self) -> bool:
        """The next step is a compressed-stage step."""
        return self.steps >= self.freeze_step

    def lr_step(self) -> float:
        """Host ``lr_step`` of the next (compressed-stage) step."""
        b1, b2 = self.betas
        return oracle.onebit_lr_step(self.lr, b1, b2, self.steps + 1, self.freeze_step)

    def hparams(self) -> dict:
        return dict(lr=self.lr, lr_step=self.lr_step(), betas=self.betas, eps=self.eps,
                    weight_decay=self.weight_decay, freeze_step=self.freeze_step,
                    step_t=self.step_t, lr_t=self.lr_t)

    def step_range(self, start, length, grad, grad_scale=1.0):
        if self.frozen:
            raise RuntimeError("1-bit Adam is past its freeze step: the sign exchange runs the "
                               "step (a dense step would write exp_avg_sq)")
        super().step_range(start, length, grad, grad_scale)

    def state_dict(self):
        return dict(super().state_dict(), kind="onebit_adam", freeze_step=self.freeze_step)

    def load_state_dict(self, sd):
        super().load_state_dict(sd)
        self.freeze_step = int(sd.get("freeze_step", self.freeze_step))


class FlatLion(_LrMixin):
    """Lion (Chen et al., "Symbolic Discovery of Optimization Algorithms", 2023): the update is
    the sign of an interpolation of the momentum and the gradient, ``p -= lr * (sign(m * beta1 +
    (1 - beta1) * g) + wd * p)``, then ``m = m * beta2 + (1 - beta2) * g``; one state buffer, half
    of Adam's.  ``step_range`` is the dense step (one HIP kernel over a flat range, the torch
    oracle on the CPU).  Under the ``vote`` codec (Distributed Lion, Liu et al. 2024) the
    exchange runs the step instead: every rank keeps its *own* ``exp_avg``, sends one bit per
    element and applies the vote (``Codec.encode_vote`` / ``decode_apply_vote``).  ``step_t`` is
    the device copy of the step count: the vote's exact-zero dither reads it, so a captured step
    dithers with the current step."""
    fusable = False
    lion = True

    def __init__(self, flat, lr=1e-4, betas=(0.9, 0.99), weight_decay=0.0):
        b1, b2 = (float(b) for b in betas)
        if not (0.0 <= b1 < 1.0 and 0.0 <= b2 < 1.0):
            raise ValueError(f"Lion's betas must lie in [0, 1), not {betas!r}")
        self.flat = flat
        self._init_lr(lr, flat.data.device)
        self.betas, self.weight_decay = (b1, b2), weight_decay
        self.exp_avg = torch.zeros_like(flat.data)
        self.steps = 0
        self.step_t = torch.zeros(1, dtype=torch.int32, device=flat.data.device) \
            if flat.data.is_cuda else None

    def hparams(self) -> dict:
        return dict(lr=self.lr, betas=self.betas, weight_decay=self.weight_decay,
                    step_t=self.step_t, lr_t=self.lr_t)

    def step_range(self, start, length, grad, grad_scale=1.0):
        b1, b2 = self.betas
        sl = slice(start, start + length)
        p, m = self.flat.data[sl], self.exp_avg[sl]
        if p.is_cuda:
            sh = self.flat.shadow[sl] if self.flat.shadow is not None else None
            ops.lion_flat(p, m, grad, self.lr, b1, b2, self.weight_decay, grad_scale, shadow=sh,
                          lr_tensor=self.lr_t)
            return
        g = grad.to(torch.float32)
        if grad_scale != 1.0:
            g = g * grad_scale
        oracle.lion_apply(p, m, g, self.lr, b1, b2, self.weight_decay)

    def step(self, grad=None, grad_scale=1.0):
        self.step_range(0, self.flat.numel, self.flat.grad if grad is None else grad, grad_scale)
        self.end_step()

    def end_step(self):
        self.steps += 1
        if self.step_t is not None:
            self.step_t.add_(1)  # on the stream: captured into the step graph

    def state_dict(self):
        return {"kind": "lion", "exp_avg": self.exp_avg, "steps": self.steps, "lr": self.lr}

    def load_state_dict(self, sd):
        self.exp_avg.copy_(sd["exp_avg"])
        self.steps = int(sd["steps"])
        if self.step_t is not None:
            self.step_t.fill_(self.steps)
        self.lr = sd.get("lr", self.lr)


class _Layerwise(_LrMixin):
    """Shared part of the layer-wise trust-ratio optimizers :class:`FlatLARS` / :class:`FlatLAMB`.

    A tensor *adapts* (takes a trust ratio) when it has two or more dimensions; biases and
    BatchNorm scales take ratio 1.  ``ratio`` (fp32, one entry per tensor in flat order) holds
    the ratios of the last step.  A step covers one bucket or the whole model
    (:meth:`step_range` with that range): on the GPU two launches (``ops.layerwise_step``), on the
    CPU the torch oracle.  The 1-based step ``t`` is read from the device counter ``step_t``, so a
    captured step replays the current step's values."""
    fusable = False
    kind = None

    def __init__(self, flat, lr, weight_decay):
        self.flat = flat
        dev = flat.data.device
        self._init_lr(lr, dev)
        self.weight_decay = weight_decay
        self.steps = 0
        self.adapts = [p.dim() >= 2 for p in flat.params]
        self.ratio = torch.ones(len(flat.params), dtype=torch.float32, device=dev)
        self.step_t = torch.zeros(1, dtype=torch.int32, device=dev) if dev.type == "cuda" else None
        # flat ranges a step may cover -> (first tensor, tensors): the whole model and each bucket
        self._ranges = {(0, flat.numel): (0, len(flat.params))}
        t0 = 0
        for b in flat.buckets:
            self._ranges[(b.start, b.length)] = (t0, len(b.params))
            t0 += len(b.params)
        self._plans = {}
        if dev.type == "cuda":
            from ..compress.plan import CHUNK

            self._adapt_t = torch.tensor(self.adapts, dtype=torch.int32, device=dev)
            self._chunk0 = [0]
            for p in flat.params:
                self._chunk0.append(self._chunk0[-1] + (p.numel() + CHUNK - 1) // CHUNK)
            self._partials = torch.zeros(2 * self._chunk0[-1], dtype=torch.float32, device=dev)

    def _range(self, start, length):
        try:
            return self._ranges[(start, length)]
        except KeyError:
            raise ValueError(f"a layer-wise step covers a bucket or the whole model (norms are "
                             f"per tensor), not the range [{start}, {start + length})") from None

    def _plan(self, start, length):
        """The range's device plan (built once): its tables and its views of ``adapt`` /
        ``ratio`` / the per-chunk partial sums."""
        lw = self._plans.get((start, length))
        if lw is None:
            from ..compress.plan import BucketPlan

            t0, nt = self._range(start, length)
            plan = BucketPlan([p.numel() for p in self.flat.params[t0:t0 + nt]],
                              [o - start for o in self.flat.offsets[t0:t0 + nt]], 1.0, start,
                              length)
            c0, c1 = self._chunk0[t0], self._chunk0[t0 + nt]
            lw = ops.LayerwisePlan(plan, self._adapt_t[t0:t0 + nt], self.ratio[t0:t0 + nt],
                                   self._partials[2 * c0:2 * c1])
            self._plans[(start, length)] = lw
        return lw

    def _tensors(self, start, length):
        t0, nt = self._range(start, length)
        return t0, [(self.flat.offsets[t] - start, self.flat.params[t].numel(), self.adapts[t])
                    for t in range(t0, t0 + nt)]

    def trust_ratio_range(self):
        """(min, max) of the last step's ratios over the adapting tensors (synchronises); None
        when no tensor adapts."""
        r = self.ratio[torch.tensor(self.adapts, dtype=torch.bool, device=self.ratio.device)]
        return (float(r.min()), float(r.max())) if r.numel() else None

    def step(self, grad=None, grad_scale=1.0):
        self.step_range(0, self.flat.numel, self.flat.grad if grad is None else grad, grad_scale)
        self.end_step()

    def end_step(self):
        self.steps += 1
        if self.step_t is not None:
            self.step_t.add_(1)  # on the stream: captured into the step graph

    def _load_common(self, sd):
        self.steps = int(sd["steps"])
        if self.step_t is not None:
            self.step_t.fill_(self.steps)
        if "ratio" in sd and sd["ratio"] is not None:
            self.ratio.copy_(sd["ratio"])
        self.lr = sd.get("lr", self.lr)
        self.weight_decay = sd.get("weight_decay", self.weight_decay)


class FlatLARS(_Layerwise):
    """LARS (You et al., 2017): per adapting tensor ``r = eta |p| / (|g| + wd |p|)`` (1 when a
    norm is zero), then :class:`FlatSGD`'s rule on ``r (g + wd p)`` with its own weight decay off
    (momentum buffer = the first such gradient, dampening, Nesterov)."""
    kind = "lars"

    def __init__(self, flat, lr=0.01, momentum=0.0, dampening=0.0, weight_decay=0.0,
                 nesterov=False, eta=0.001):
        if nesterov and (momentum <= 0 or dampening != 0):
            raise ValueError("Nesterov momentum requires a momentum and zero dampening")
        super().__init__(flat, lr, weight_decay)
        self.momentum, self.dampening, self.nesterov, self.eta = momentum, dampening, nesterov, eta
        self.mom = torch.zeros_like(flat.data)

    @property
    def first(self) -> bool:
        return self.steps == 0

    def step_range(self, start, length, grad, grad_scale=1.0):
        sl = slice(start, start + length)
        p, m = self.flat.data[sl], self.mom[sl]
        if p.is_cuda:
            sh = self.flat.shadow[sl] if self.flat.shadow is not None else None
            ops.layerwise_step(self._plan(start, length), "lars", p, grad, m, lr=self.lr,
                               weight_decay=self.weight_decay, grad_scale=grad_scale,
                               eta=self.eta, momentum=self.momentum, dampening=self.dampening,
                               nesterov=self.nesterov, first=self.first, step=self.step_t,
                               lr_tensor=self.lr_t, shadow=sh)
            return
        t0, tensors = self._tensors(start, length)
        g = grad.to(torch.float32) * grad_scale
        self.ratio[t0:t0 + len(tensors)] = oracle.lars_apply(
            p, m, g, tensors, self.lr, self.momentum, self.dampening, self.weight_decay,
            self.nesterov, self.first, self.eta)

    def state_dict(self):
        return {"kind": "lars", "mom": self.mom, "steps": self.steps, "ratio": self.ratio,
                "lr": self.lr, "momentum": self.momentum, "dampening": self.dampening,
                "weight_decay": self.weight_decay, "nesterov": self.nesterov, "eta": self.eta}

    def load_state_dict(self, sd):
        self.mom.copy_(sd["mom"])
        self._load_common(sd)
        for k in ("momentum", "dampening", "nesterov", "eta"):
            if k in sd:
                setattr(self, k, sd[k])


class FlatLAMB(_Layerwise):
    """LAMB (You et al., ICLR 2020): Adam's moments with bias correction, ``u = m^ / (sqrt(v^) +
    eps) + wd p``, per adapting tensor ``r = |p| / |u|`` (1 when a norm is zero), ``p -= lr r u``.
    No clamp on ``|p|`` and no gradient clipping."""
    kind = "lamb"

    def __init__(self, flat, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0):
        super().__init__(flat, lr, weight_decay)
        self.betas, self.eps = betas, eps
        self.exp_avg = torch.zeros_like(flat.data)
        self.exp_avg_sq = torch.zeros_like(flat.data)

    def step_range(self, start, length, grad, grad_scale=1.0):
        sl = slice(start, start + length)
        p, m, v = self.flat.data[sl], self.exp_avg[sl], self.exp_avg_sq[sl]
        if p.is_cuda:
            sh = self.flat.shadow[sl] if self.flat.shadow is not None else None
            ops.layerwise_step(self._plan(start, length), "lamb", p, grad, m, v, lr=self.lr,
                               weight_decay=self.weight_decay, grad_scale=grad_scale,
                               betas=self.betas, eps=self.eps, t=self.steps + 1,
                               step=self.step_t, lr_tensor=self.lr_t, shadow=sh)
            return
        t0, tensors = self._tensors(start, length)
        g = grad.to(torch.float32) * grad_scale
        b1, b2 = self.betas
        self.ratio[t0:t0 + len(tensors)] = oracle.lamb_apply(
            p, m, v, g, tensors, self.lr, b1, b2, self.eps, self.weight_decay, self.steps + 1)

    def state_dict(self):
        return {"kind": "lamb", "exp_avg": self.exp_avg, "exp_avg_sq": self.exp_avg_sq,
                "steps": self.steps, "ratio": self.ratio, "lr": self.lr,
                "weight_decay": self.weight_decay}

    def load_state_dict(self, sd):
        self.exp_avg.copy_(sd["exp_avg"])
        self.exp_avg_sq.copy_(sd["exp_avg_sq"])
        self._load_common(sd)


class FlatOnebitLamb(FlatLAMB):
    """1-bit LAMB (Li et al., 2021; DeepSpeed ``OnebitLamb``).  Steps 1..``freeze_step`` are
    :class:`FlatLAMB` on the dense averaged gradient; :meth:`end_step` also keeps per tensor
    ``coeff_ema = coeff_beta * coeff_ema + (1 - coeff_beta) * ratio``.  From then on (``frozen``)
    ``exp_avg_sq`` is never written again and the exchange, not :meth:`step_range`, runs the
    step (``Codec.encode_momentum`` with weight decay 0 / ``decode_apply_onebit_lamb``,
    ``compress/oracle.py onebit_lamb_apply``): the decode writes the averaged momentum into
    ``exp_avg``, moves ``exp_avg_sq_fresh`` with the gradient the momentum implies, and steps with
    ``ratio = r_frozen * factor``, the factor following ``max (sqrt(v) + eps) / (sqrt(v_fresh) +
    eps)`` inside ``[factor_min, factor_max]`` and within ``factor_threshold`` of the last one.

    The freeze (``exp_avg_sq_fresh = exp_avg_sq``, ``r_frozen = coeff_ema / (1 - coeff_beta^
    freeze_step)``, ``last_factor = 1``) is written at the end of *every* warm-up step, with
    stream-ordered copies and no branch on the step count: a captured warm-up step replays it,
    and what step ``freeze_step`` leaves is the freeze.  ``last_factor`` is kept as two rows: step
    ``t`` reads row ``(t - 1) & 1`` and writes row ``t & 1``.  The state is the same on every
    rank; the error-feedback residual lives in the exchange."""
    onebit = True
    onebit_kind = "lamb"

    def __init__(self, flat, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0,
                 freeze_step=None, coeff_beta=0.9, factor_min=0.5, factor_max=4.0,
                 factor_threshold=0.1):
        if freeze_step is None or int(freeze_step) < 1:
            raise ValueError("1-bit LAMB needs freeze_step >= 1 (the dense warm-up's length)")
        if not (0.0 <= coeff_beta < 1.0 and 0.0 < factor_min <= 1.0 <= factor_max
                and 0.0 <= factor_threshold < 1.0):
            raise ValueError("1-bit LAMB needs coeff_beta in [0, 1), factor_min <= 1 <= "
                             "factor_max and factor_threshold in [0, 1)")
        super().__init__(flat, lr=lr, betas=betas, eps=eps, weight_decay=weight_decay)
        self.freeze_step = int(freeze_step)
        self.coeff_beta = float(coeff_beta)
        self.factor_min, self.factor_max = float(factor_min), float(factor_max)
        self.factor_threshold = float(factor_threshold)
        self.exp_avg_sq_fresh = torch.zeros_like(flat.data)
        self.coeff_ema = torch.zeros_like(self.ratio)
        self.r_frozen = torch.zeros_like(self.ratio)
        self._factors = torch.ones(2, self.ratio.numel(), dtype=torch.float32,
                                   device=self.ratio.device)
        self._tables = {}

    @property
    def frozen(self) -> bool:
        """The next step is a compressed-stage step."""
        return self.steps >= self.freeze_step

    @property
    def last_factor(self) -> torch.Tensor:
        """The factors the last step left (the row of its parity)."""
        return self._factors[self.steps & 1]

    def hparams(self, start=None, length=None) -> dict:
        """The decode's arguments; with a bucket's range also its per-tensor state: the
        ``(offset, numel, adapts)`` rows, views of ``r_frozen`` / ``ratio`` / the two factor rows,
        and (GPU) ``tables(dp)``, the device tables over the codec's decode plan."""
        hp = dict(lr=self.lr, betas=self.betas, eps=self.eps, weight_decay=self.weight_decay,
                  freeze_step=self.freeze_step, t=self.steps + 1, factor_min=self.factor_min,
                  factor_max=self.factor_max, factor_threshold=self.factor_threshold,
                  step_t=self.step_t, lr_t=self.lr_t)
        if start is not None:
            t0, tensors = self._tensors(start, length)
            sl = slice(t0, t0 + len(tensors))
            hp.update(tensors=tensors, r_frozen=self.r_frozen[sl], ratio=self.ratio[sl],
                      factors=self._factors[:, sl],
                      tables=lambda dp: self._bucket_tables(dp, start, length))
        return hp

    def step_range(self, start, length, grad, grad_scale=1.0):
        if self.frozen:
            raise RuntimeError("1-bit LAMB is past its freeze step: the sign exchange runs the "
                               "step (a dense step would write exp_avg_sq)")
        super().step_range(start, length, grad, grad_scale)

    def _bucket_tables(self, dp, start, length):
        lt = self._tables.get((start, length))
        if lt is None:
            t0, nt = self._range(start, length)
            c0 = self._chunk0[t0]
            lt = ops.OnebitLambTables(dp, self._adapt_t[t0:t0 + nt], self.r_frozen[t0:t0 + nt],
                                      self._factors[:, t0:t0 + nt], self.ratio[t0:t0 + nt],
                                      self._partials[c0:c0 + dp.plan.num_chunks])
            self._tables[(start, length)] = lt
        return lt

    def end_step(self):
        if not self.frozen:  # a warm-up step just ran: self.ratio holds its trust ratios
            self.coeff_ema.mul_(self.coeff_beta).add_(self.ratio * (1.0 - self.coeff_beta))
            torch.div(self.coeff_ema, 1.0 - self.coeff_beta ** self.freeze_step,
                      out=self.r_frozen)
            self.exp_avg_sq_fresh.copy_(self.exp_avg_sq)
        super().end_step()

    def state_dict(self):
        return dict(super().state_dict(), kind="onebit_lamb", freeze_step=self.freeze_step,
                    exp_avg_sq_fresh=self.exp_avg_sq_fresh, coeff_ema=self.coeff_ema,
                    r_frozen=self.r_frozen, last_factor=self._factors,
                    coeff_beta=self.coeff_beta, factor_min=self.factor_min,
                    factor_max=self.factor_max, factor_threshold=self.factor_threshold)

    def load_state_dict(self, sd):
        super().load_state_dict(sd)
        self.exp_avg_sq_fresh.copy_(sd["exp_avg_sq_fresh"])
        self.coeff_ema.copy_(sd["coeff_ema"])
        self.r_frozen.copy_(sd["r_frozen"])
        self._factors.copy_(sd["last_factor"])
        self.freeze_step = int(sd.get("freeze_step", self.freeze_step))
        for k in ("coeff_beta", "factor_min", "factor_max", "factor_threshold"):
            if k in sd:
                setattr(self, k, float(sd[k]))


def make_optimizer(name, flat, **kw):
    name = name.lower()
    if name == "onebit_lamb":
        return FlatOnebitLamb(flat, lr=kw.get("lr", 1e-3),
                              weight_decay=kw.get("weight_decay", 0.0), eps=kw.get("eps", 1e-8),
                              freeze_step=kw.get("freeze_step"))
    if name == "lars":
        return FlatLARS(flat, eta=kw.get("eta", 0.001),
                        **{k: v for k, v in kw.items()
                           if k in ("lr", "momentum", "dampening", "weight_decay", "nesterov")})
    if name == "lamb":
        return FlatLAMB(flat, lr=kw.get("lr", 1e-3), weight_decay=kw.get("weight_decay", 0.0),
                        eps=kw.get("eps", 1e-8))
    if name == "sgd":
        return FlatSGD(flat, **{k: v for k, v in kw.items()
                                if k in ("lr", "momentum", "dampening", "weight_decay",
                                         "nesterov")})
    if name in ("adam", "amsgrad"):
        return FlatAdam(flat, lr=kw.get("lr", 1e-3), weight_decay=kw.get("weight_decay", 0.0),
                        eps=kw.get("eps", 1e-8),
                        amsgrad=(name == "amsgrad") or kw.get("amsgrad", False))
    if name == "lion":
        return FlatLion(flat, lr=kw.get("lr", 1e-4), betas=kw.get("betas") or (0.9, 0.99),
                        weight_decay=kw.get("weight_decay", 0.0))
    if name == "onebit_adam":
        return FlatOnebitAdam(flat, lr=kw.get("lr", 1e-3),
                              weight_decay=kw.get("weight_decay", 0.0), eps=kw.get("eps", 1e-8),
                              amsgrad=kw.get("amsgrad", False),
                              freeze_step=kw.get("freeze_step"))
    raise ValueError(f"unknown optimizer {name!r}")
