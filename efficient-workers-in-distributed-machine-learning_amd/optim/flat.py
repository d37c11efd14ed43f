"""Optimizers over the flat parameter buffer with *explicit* gradients.

Parity: ``optim/sgd.py:11-91`` (SGD whose ``step(grads=...)`` takes the averaged gradient received
from the server; momentum buffer initialised to the first gradient, dampening, Nesterov, weight
decay) and ``optim/adam.py:12-94`` (Adam/AMSGrad with explicit gradients).  The reference loops
over parameter tensors; these run one HIP kernel over a flat range (``ops.sgd_flat`` /
``ops.adam_flat``), and the top-k / QSGD exchanges fuse the SGD update into their decode kernel
(``Codec.decode_apply_sgd``) so the averaged gradient never round-trips through HBM.

Every class derives from :class:`_Flat` (the learning rate, the step counters, the whole-model
step, the checkpoint); the ones whose step covers whole tensors from :class:`_PerTensor`; the
three whose state the whole model's plan lays out from :class:`_Factored`.  ``optim/kinds.py``
names the classes and their options for the command line, the trainer and ``make_optimizer``.
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


# how a saved hyper-parameter is read back from a checkpoint (every other one as it is)
_READ = {"freeze_step": int, "seed": int, "coeff_beta": float, "factor_min": float,
         "factor_max": float, "factor_threshold": float}


class _Flat:
    """What every optimizer here shares.  ``lr`` is a host value mirrored into ``lr_t`` (device)
    on the GPU; ``steps`` counts the finished steps, and ``step_t`` is its device copy: the
    kernels derive the bias correction (the dither, the refresh) from it, so a captured HIP graph
    replays the current step's values, not the capture step's.  A subclass gives
    :meth:`step_range` and names its checkpoint: ``_KIND``, the state tensors ``_STATE`` (one
    that is ``None`` is not loaded; one in ``_OPTIONAL`` may be missing from the checkpoint) and
    the saved hyper-parameters ``_HPARAMS`` (each loaded when the checkpoint has it)."""
    fusable = False
    _KIND = None
    _STATE = ()
    _OPTIONAL = ()
    _HPARAMS = ()
    _COUNTER = True  # keeps the device step counter

    def _init(self, flat, lr):
        self.flat = flat
        dev = flat.data.device
        self._lr_dev = DeviceScalar(lr, dev) if dev.type == "cuda" else None
        self._lr = float(lr)
        self.steps = 0
        self.step_t = torch.zeros(1, dtype=torch.int32, device=dev) \
            if self._COUNTER and dev.type == "cuda" else None
        return dev

    @property
    def lr(self) -> float:
        return self._lr

    @lr.setter
    def lr(self, value: float):
        self._lr = float(value)
        if self._lr_dev is not None:
            self._lr_dev.set(self._lr)

    @property
    def lr_t(self):
        return None if self._lr_dev is None else self._lr_dev.t

    def _shadow(self, start, length):
        """The range's view of the bf16 shadow parameters (None without them)."""
        sh = self.flat.shadow
        return None if sh is None else sh[start:start + length]

    def step(self, grad: torch.Tensor = None, grad_scale: float = 1.0):
        """Whole-model step (``grad`` defaults to the flat gradient buffer)."""
        self.step_range(0, self.flat.numel, self.flat.grad if grad is None else grad, grad_scale)
        self.end_step()

    def end_step(self):
        self.steps += 1
        if self.step_t is not None:
            self.step_t.add_(1)  # on the stream: captured into the step graph

    def state_dict(self):
        return {"kind": self._KIND, **{k: getattr(self, k) for k in self._STATE},
                "steps": self.steps, "lr": self.lr,
                **{k: getattr(self, k) for k in self._HPARAMS}}

    def load_state_dict(self, sd):
        for k in self._STATE:
            t = getattr(self, k)
            if t is not None and not (k in self._OPTIONAL and sd.get(k) is None):
                t.copy_(sd[k])
        self.steps = int(sd["steps"])
        if self.step_t is not None:
            self.step_t.fill_(self.steps)
        self.lr = sd.get("lr", self.lr)
        for k in self._HPARAMS:
            if k in sd:
                setattr(self, k, _READ[k](sd[k]) if k in _READ else sd[k])


class _StateBytes:
    def state_bytes(self) -> int:
        """Bytes of optimizer state (the tensors of ``_STATE`` that exist)."""
        return sum(t.numel() * t.element_size()
                   for t in (getattr(self, k) for k in self._STATE) if t is not None)


class _PerTensor(_Flat):
    """An optimizer with per-tensor quantities (norms, blocks, factors): a step covers one bucket
    or the whole model, never another range.  ``_COVERS`` words the refusal; :meth:`_plan` caches
    what :meth:`_make_plan` builds for a range from its ``BucketPlan``."""
    _COVERS = None  # ("a layer-wise", "norms are")

    def _init(self, flat, lr):
        dev = super()._init(flat, lr)
        # flat ranges a step may cover -> (first tensor, tensors): the whole model and each bucket
        self._ranges = {(0, flat.numel): (0, len(flat.params))}
        t0 = 0
        for b in flat.buckets:
            self._ranges[(b.start, b.length)] = (t0, len(b.params))
            t0 += len(b.params)
        self._plans = {}
        return dev

    def _range(self, start, length):
        try:
            return self._ranges[(start, length)]
        except KeyError:
            step, per = self._COVERS
            raise ValueError(f"{step} step covers a bucket or the whole model ({per} per "
                             f"tensor), not the range [{start}, {start + length})") from None

    def _chunk_starts(self):
        """The first chunk of every tensor when each starts a chunk of its own, and the total."""
        from ..compress.plan import CHUNK

        c0 = [0]
        for p in self.flat.params:
            c0.append(c0[-1] + (p.numel() + CHUNK - 1) // CHUNK)
        return c0

    def _bucket_plan(self, start, length):
        """The ``BucketPlan`` of a range, its tensors' offsets counted from ``start``."""
        from ..compress.plan import BucketPlan

        t0, nt = self._range(start, length)
        return BucketPlan([p.numel() for p in self.flat.params[t0:t0 + nt]],
                          [o - start for o in self.flat.offsets[t0:t0 + nt]], 1.0, start, length)

    def _plan(self, start, length):
        """The range's device plan (built once)."""
        got = self._plans.get((start, length))
        if got is None:
            t0, nt = self._range(start, length)
            got = self._plans[(start, length)] = self._make_plan(
                self._bucket_plan(start, length), t0, nt)
        return got


class FlatSGD(_Flat):
    fusable = True
    _KIND = "sgd"
    _STATE = ("mom",)
    _HPARAMS = ("momentum", "dampening", "weight_decay", "nesterov")
    _COUNTER = False

    def __init__(self, flat, lr=0.01, momentum=0.0, dampening=0.0, weight_decay=0.0,
                 nesterov=False):
        if nesterov and (momentum <= 0 or dampening != 0):
            raise ValueError("Nesterov momentum requires a momentum and zero dampening")
        self._init(flat, lr)
        self.momentum, self.dampening = momentum, dampening
        self.weight_decay, self.nesterov = weight_decay, nesterov
        self.mom = torch.zeros_like(flat.data)

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
            ops.sgd_flat(p, m, grad, self.lr, self.momentum, self.dampening, self.weight_decay,
                         grad_scale, self.nesterov, self.first,
                         shadow=self._shadow(start, length), lr_tensor=self.lr_t)
            return
        g = grad.to(torch.float32)
        if grad_scale != 1.0:
            g = g * grad_scale
        oracle.sgd_apply(p, m, g, self.lr, self.momentum, self.dampening, self.weight_decay,
                         self.nesterov, self.first)

    def step_bucket_ptrs(self, b, dp, grads, grad_scale: float = 1.0):
        """SGD of bucket ``b`` from its per-tensor gradients ``grads`` (pointer mode), one
        launch; no :meth:`end_step`."""
        p = self.flat.data_view(b)
        m = self.mom[b.start:b.start + b.length]
        ops.sgd_ptrs(dp, grads, p, m, self.lr, self.momentum, self.dampening, self.weight_decay,
                     grad_scale, self.nesterov, self.first, shadow=self.flat.shadow_view(b),
                     lr_tensor=self.lr_t)


class FlatAdam(_Flat):
    _KIND = "adam"
    _STATE = ("exp_avg", "exp_avg_sq", "max_exp_avg_sq")
    _OPTIONAL = ("max_exp_avg_sq",)

    def __init__(self, flat, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0,
                 amsgrad=False):
        self._init(flat, lr)
        self.betas, self.eps = betas, eps
        self.weight_decay, self.amsgrad = weight_decay, amsgrad
        self.exp_avg = torch.zeros_like(flat.data)
        self.exp_avg_sq = torch.zeros_like(flat.data)
        self.max_exp_avg_sq = torch.zeros_like(flat.data) if amsgrad else None

    def step_range(self, start, length, grad, grad_scale=1.0):
        t = self.steps + 1
        b1, b2 = self.betas
        sl = slice(start, start + length)
        p = self.flat.data[sl]
        vmax = self.max_exp_avg_sq[sl] if self.amsgrad else None
        if p.is_cuda:
            lr_step = self.lr * math.sqrt(1 - b2 ** t) / (1 - b1 ** t)
            ops.adam_flat(p, self.exp_avg[sl], self.exp_avg_sq[sl], vmax, grad, lr_step, b1, b2,
                          self.eps, self.weight_decay, grad_scale, self.amsgrad,
                          shadow=self._shadow(start, length), step=self.step_t, lr=self.lr,
                          lr_tensor=self.lr_t)
            return
        g = grad.to(torch.float32) * grad_scale
        oracle.adam_apply(p, self.exp_avg[sl], self.exp_avg_sq[sl],
                          vmax if vmax is not None else torch.empty(0), g, self.lr, b1, b2,
                          self.eps, self.weight_decay, t, self.amsgrad)


class FlatAdam8bit(_PerTensor, _StateBytes):
    """8-bit Adam (Dettmers et al., ICLR 2022): :class:`FlatAdam`'s rule with both moments kept
    as one byte per element (``code_m`` / ``code_v``, indexed like ``flat.data``) plus one fp32
    absmax per 256-element block of a tensor (``absmax_m`` / ``absmax_v``, 32 slots per global
    8192-element chunk), about 2.03 B of state per element instead of 8
    (``compress/oracle.py adam8_apply`` defines the format).  A step covers one bucket or the
    whole model, as blocks are counted per tensor: one HIP kernel on the GPU
    (``ops.adam8_step``), the torch oracle on the CPU.  No AMSGrad."""
    _KIND = "adam8bit"
    _STATE = ("code_m", "code_v", "absmax_m", "absmax_v")
    _COVERS = ("an 8-bit Adam", "blocks are")

    def __init__(self, flat, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0):
        dev = self._init(flat, lr)
        self.betas, self.eps, self.weight_decay = betas, eps, weight_decay
        self._chunk0 = self._chunk_starts()
        self.code_m, self.code_v, self.absmax_m, self.absmax_v = oracle.adam8_state(
            flat.data.numel(), self._chunk0[-1], dev)

    def _make_plan(self, plan, t0, nt):
        """The range's chunk table and absmax views."""
        s0, s1 = (oracle.ADAM8_SLOTS * self._chunk0[t] for t in (t0, t0 + nt))
        return ops.Adam8Plan(plan, self.absmax_m[s0:s1], self.absmax_v[s0:s1])

    def step_range(self, start, length, grad, grad_scale=1.0):
        t0, nt = self._range(start, length)
        sl = slice(start, start + length)
        p, cm, cv = self.flat.data[sl], self.code_m[sl], self.code_v[sl]
        if p.is_cuda:
            ops.adam8_step(self._plan(start, length), p, grad, cm, cv,
                           lr_step=oracle.adam8_lr_step(self.lr, *self.betas, self.steps + 1),
                           betas=self.betas, eps=self.eps, weight_decay=self.weight_decay,
                           grad_scale=grad_scale, shadow=self._shadow(start, length),
                           step=self.step_t, lr=self.lr, lr_tensor=self.lr_t)
            return
        blocks = [(self.flat.offsets[t] - start, self.flat.params[t].numel(),
                   oracle.ADAM8_SLOTS * self._chunk0[t]) for t in range(t0, t0 + nt)]
        g = grad.to(torch.float32) * grad_scale
        oracle.adam8_apply(p, cm, cv, self.absmax_m, self.absmax_v, g, blocks, self.lr,
                           *self.betas, self.eps, self.weight_decay, self.steps + 1)


class FlatOnebitAdam(FlatAdam):
    """1-bit Adam (Tang et al., ICML 2021; DeepSpeed ``OnebitAdam``).  Steps 1..``freeze_step`` are
    :class:`FlatAdam` on the dense averaged gradient.  From then on (``frozen``) ``exp_avg_sq`` is
    never written again and the exchange, not :meth:`step_range`, runs the step: every rank
    sign-compresses its error-compensated momentum candidate, and the decode writes the average
    into ``exp_avg`` and applies ``p -= lr_step * exp_avg / (sqrt(exp_avg_sq) + eps)``
    (``Codec.encode_momentum`` / ``decode_apply_onebit``).  The error-feedback residual is per-rank
    state and lives in the exchange; this optimizer's state is the same on every rank."""
    onebit = True
    _KIND = "onebit_adam"
    _HPARAMS = ("freeze_step",)

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


class FlatLion(_Flat):
    """Lion (Chen et al., "Symbolic Discovery of Optimization Algorithms", 2023): the update is
    the sign of an interpolation of the momentum and the gradient, ``p -= lr * (sign(m * beta1 +
    (1 - beta1) * g) + wd * p)``, then ``m = m * beta2 + (1 - beta2) * g``; one state buffer, half
    of Adam's.  ``step_range`` is the dense step (one HIP kernel over a flat range, the torch
    oracle on the CPU).  Under the ``vote`` codec (Distributed Lion, Liu et al. 2024) the
    exchange runs the step instead: every rank keeps its *own* ``exp_avg``, sends one bit per
    element and applies the vote (``Codec.encode_vote`` / ``decode_apply_vote``).  ``step_t`` is
    the device copy of the step count: the vote's exact-zero dither reads it, so a captured step
    dithers with the current step."""
    lion = True
    _KIND = "lion"
    _STATE = ("exp_avg",)

    def __init__(self, flat, lr=1e-4, betas=(0.9, 0.99), weight_decay=0.0):
        b1, b2 = (float(b) for b in betas)
        if not (0.0 <= b1 < 1.0 and 0.0 <= b2 < 1.0):
            raise ValueError(f"Lion's betas must lie in [0, 1), not {betas!r}")
        self._init(flat, lr)
        self.betas, self.weight_decay = (b1, b2), weight_decay
        self.exp_avg = torch.zeros_like(flat.data)

    def hparams(self) -> dict:
        return dict(lr=self.lr, betas=self.betas, weight_decay=self.weight_decay,
                    step_t=self.step_t, lr_t=self.lr_t)

    def step_range(self, start, length, grad, grad_scale=1.0):
        b1, b2 = self.betas
        sl = slice(start, start + length)
        p, m = self.flat.data[sl], self.exp_avg[sl]
        if p.is_cuda:
            ops.lion_flat(p, m, grad, self.lr, b1, b2, self.weight_decay, grad_scale,
                          shadow=self._shadow(start, length), lr_tensor=self.lr_t)
            return
        g = grad.to(torch.float32)
        if grad_scale != 1.0:
            g = g * grad_scale
        oracle.lion_apply(p, m, g, self.lr, b1, b2, self.weight_decay)


class _Layerwise(_PerTensor):
    """Shared part of the layer-wise trust-ratio optimizers :class:`FlatLARS` / :class:`FlatLAMB`.

    A tensor *adapts* (takes a trust ratio) when it has two or more dimensions; biases and
    BatchNorm scales take ratio 1.  ``ratio`` (fp32, one entry per tensor in flat order) holds
    the ratios of the last step.  A step covers one bucket or the whole model
    (:meth:`step_range` with that range): on the GPU two launches (``ops.layerwise_step``), on the
    CPU the torch oracle.  The 1-based step ``t`` is read from the device counter ``step_t``, so a
    captured step replays the current step's values."""
    kind = None
    _OPTIONAL = ("ratio",)
    _COVERS = ("a layer-wise", "norms are")

    def __init__(self, flat, lr, weight_decay):
        dev = self._init(flat, lr)
        self.weight_decay = weight_decay
        self.adapts = [p.dim() >= 2 for p in flat.params]
        self.ratio = torch.ones(len(flat.params), dtype=torch.float32, device=dev)
        if dev.type == "cuda":
            self._adapt_t = torch.tensor(self.adapts, dtype=torch.int32, device=dev)
            self._chunk0 = self._chunk_starts()
            self._partials = torch.zeros(2 * self._chunk0[-1], dtype=torch.float32, device=dev)

    def _make_plan(self, plan, t0, nt):
        """The range's tables and its views of ``adapt`` / ``ratio`` / the per-chunk partial
        sums."""
        c0, c1 = self._chunk0[t0], self._chunk0[t0 + nt]
        return ops.LayerwisePlan(plan, self._adapt_t[t0:t0 + nt], self.ratio[t0:t0 + nt],
                                 self._partials[2 * c0:2 * c1])

    def _tensors(self, start, length):
        t0, nt = self._range(start, length)
        return t0, [(self.flat.offsets[t] - start, self.flat.params[t].numel(), self.adapts[t])
                    for t in range(t0, t0 + nt)]

    def trust_ratio_range(self):
        """(min, max) of the last step's ratios over the adapting tensors (synchronises); None
        when no tensor adapts."""
        r = self.ratio[torch.tensor(self.adapts, dtype=torch.bool, device=self.ratio.device)]
        return (float(r.min()), float(r.max())) if r.numel() else None


class FlatLARS(_Layerwise):
    """LARS (You et al., 2017): per adapting tensor ``r = eta |p| / (|g| + wd |p|)`` (1 when a
    norm is zero), then :class:`FlatSGD`'s rule on ``r (g + wd p)`` with its own weight decay off
    (momentum buffer = the first such gradient, dampening, Nesterov)."""
    kind = _KIND = "lars"
    _STATE = ("mom", "ratio")
    _HPARAMS = ("momentum", "dampening", "weight_decay", "nesterov", "eta")

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
            ops.layerwise_step(self._plan(start, length), "lars", p, grad, m, lr=self.lr,
                               weight_decay=self.weight_decay, grad_scale=grad_scale,
                               eta=self.eta, momentum=self.momentum, dampening=self.dampening,
                               nesterov=self.nesterov, first=self.first, step=self.step_t,
                               lr_tensor=self.lr_t, shadow=self._shadow(start, length))
            return
        t0, tensors = self._tensors(start, length)
        g = grad.to(torch.float32) * grad_scale
        self.ratio[t0:t0 + len(tensors)] = oracle.lars_apply(
            p, m, g, tensors, self.lr, self.momentum, self.dampening, self.weight_decay,
            self.nesterov, self.first, self.eta)


class FlatLAMB(_Layerwise):
    """LAMB (You et al., ICLR 2020): Adam's moments with bias correction, ``u = m^ / (sqrt(v^) +
    eps) + wd p``, per adapting tensor ``r = |p| / |u|`` (1 when a norm is zero), ``p -= lr r u``.
    No clamp on ``|p|`` and no gradient clipping."""
    kind = _KIND = "lamb"
    _STATE = ("exp_avg", "exp_avg_sq", "ratio")
    _HPARAMS = ("weight_decay",)

    def __init__(self, flat, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0):
        super().__init__(flat, lr, weight_decay)
        self.betas, self.eps = betas, eps
        self.exp_avg = torch.zeros_like(flat.data)
        self.exp_avg_sq = torch.zeros_like(flat.data)

    def step_range(self, start, length, grad, grad_scale=1.0):
        sl = slice(start, start + length)
        p, m, v = self.flat.data[sl], self.exp_avg[sl], self.exp_avg_sq[sl]
        if p.is_cuda:
            ops.layerwise_step(self._plan(start, length), "lamb", p, grad, m, v, lr=self.lr,
                               weight_decay=self.weight_decay, grad_scale=grad_scale,
                               betas=self.betas, eps=self.eps, t=self.steps + 1,
                               step=self.step_t, lr_tensor=self.lr_t,
                               shadow=self._shadow(start, length))
            return
        t0, tensors = self._tensors(start, length)
        g = grad.to(torch.float32) * grad_scale
        b1, b2 = self.betas
        self.ratio[t0:t0 + len(tensors)] = oracle.lamb_apply(
            p, m, v, g, tensors, self.lr, b1, b2, self.eps, self.weight_decay, self.steps + 1)


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
    _KIND = "onebit_lamb"
    _STATE = FlatLAMB._STATE + ("exp_avg_sq_fresh", "coeff_ema", "r_frozen")
    _HPARAMS = FlatLAMB._HPARAMS + ("freeze_step", "coeff_beta", "factor_min", "factor_max",
                                    "factor_threshold")

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
        return dict(super().state_dict(), last_factor=self._factors)  # both rows

    def load_state_dict(self, sd):
        super().load_state_dict(sd)
        self._factors.copy_(sd["last_factor"])


class FlatMuon(_Layerwise):
    """Muon (Jordan et al., 2024): ``mom = momentum * mom + g`` and ``u = mom`` (Nesterov: ``g +
    momentum * mom``) on every tensor, with no first-step special case.  A tensor that adapts
    (``dim() >= 2``, viewed as ``[shape[0], numel / shape[0]]``) steps by ``u`` orthogonalised
    with ``ns_steps`` Newton-Schulz iterations (``compress/oracle.py muon_orthogonalize``), ``p =
    p (1 - lr wd) - lr sqrt(max(1, n / m)) O``; the others take momentum SGD at ``lr_aux = lr *
    aux_lr / (the lr at construction)``, so a schedule moves both rates together.  On the GPU a
    step is ``ops.muon_step`` (``csrc/muon.hip``), on the CPU the torch oracle."""
    kind = _KIND = "muon"
    _STATE = ("mom",)
    _HPARAMS = ("momentum", "weight_decay", "nesterov", "ns_steps", "ns_dtype", "aux_ratio")

    def __init__(self, flat, lr=0.02, momentum=0.95, weight_decay=0.0, nesterov=False,
                 ns_steps=5, ns_dtype="fp32", aux_lr=None):
        if not 1 <= int(ns_steps) <= 10:
            raise ValueError(f"Muon takes 1..10 Newton-Schulz steps, not {ns_steps!r}")
        if ns_dtype not in oracle.MUON_NS_DTYPES:
            raise ValueError(f"Muon's Newton-Schulz dtype is fp32 or bf16, not {ns_dtype!r}")
        if not lr > 0 or (aux_lr is not None and not aux_lr > 0):
            raise ValueError("Muon needs lr > 0 and aux_lr > 0")
        super().__init__(flat, lr, weight_decay)
        self.momentum, self.nesterov = momentum, nesterov
        self.ns_steps, self.ns_dtype = int(ns_steps), ns_dtype
        self.aux_ratio = 1.0 if aux_lr is None else float(aux_lr) / float(lr)
        self.mom = torch.zeros_like(flat.data)
        self.rows = [p.shape[0] if a else 0 for p, a in zip(flat.params, self.adapts)]
        self._ws = None
        if flat.data.is_cuda:  # every bucket's plan now, so the workspace fits the largest
            plans = [self._plan(b.start, b.length) for b in flat.buckets]
            self._ws = ops.MuonWorkspace([mp for mp, _ in plans], flat.data.device)
            for key, (mp, _) in list(self._plans.items()):
                self._plans[key] = (mp, self._ws)

    def trust_ratio_range(self):
        return None  # no trust ratios

    def _make_plan(self, plan, t0, nt):
        """The range's device plan and workspace.  The whole model steps in the buckets'
        workspace when it fits and in one of its own otherwise."""
        dev = self.flat.data.device
        mp = ops.MuonPlan(plan, self.rows[t0:t0 + nt]).to(dev)
        ws = self._ws
        if ws is not None and not ws.fits(mp):
            ws = ops.MuonWorkspace([mp], dev)
        return mp, ws

    def step_range(self, start, length, grad, grad_scale=1.0):
        sl = slice(start, start + length)
        p, m = self.flat.data[sl], self.mom[sl]
        hp = dict(lr=self.lr, aux_ratio=self.aux_ratio, momentum=self.momentum,
                  weight_decay=self.weight_decay, nesterov=self.nesterov,
                  ns_steps=self.ns_steps, ns_dtype=self.ns_dtype)
        if p.is_cuda:
            mp, ws = self._plan(start, length)
            c0 = self._chunk0[self._range(start, length)[0]]
            ops.muon_step(mp, ws, p, grad, m, self._partials[c0:c0 + mp.plan.num_chunks],
                          grad_scale=grad_scale, lr_tensor=self.lr_t,
                          shadow=self._shadow(start, length), **hp)
            return
        t0, tensors = self._tensors(start, length)
        rows = [(off, n, self.rows[t0 + i]) for i, (off, n, _) in enumerate(tensors)]
        oracle.muon_apply(p, m, grad.to(torch.float32) * grad_scale, rows, **hp)


class _Factored(_PerTensor, _StateBytes):
    """Shared part of :class:`FlatAdafactor`, :class:`FlatGalore` and :class:`FlatApollo`, whose
    state per tensor depends on the tensor's shape.  ``rows[t]`` is ``shape[0]`` of a tensor with
    ``dim() >= 2`` and 0 of a vector.  The whole model's plan (``_whole``) lays the state out; a
    bucket's plan sees views of it: ``_LAYOUT`` names, per state tensor of that kind, the plan's
    list of per-tensor offsets (with the total at its end) and the floats per unit of it.  A
    subclass gives ``_LAYOUT``, :meth:`_new_plan`, :meth:`_hp` and :meth:`_tensors`; its kernels
    and oracle are ``ops.<kind>_step`` / ``ops.<Kind>Workspace`` and ``oracle.<kind>_apply``."""
    _LAYOUT = ()
    _ORACLE_ONLY = ()  # attributes the oracle takes on top of _hp() (the kernels read the plan's)

    def _init(self, flat, lr):
        dev = super()._init(flat, lr)
        self.rows = [p.shape[0] if p.dim() >= 2 else 0 for p in flat.params]
        self._whole = self._new_plan(self._bucket_plan(0, flat.numel), 0, len(flat.params))
        for name, offsets, per in self._LAYOUT:
            setattr(self, name, torch.zeros(per * getattr(self._whole, offsets)[-1],
                                            dtype=torch.float32, device=dev))
        self._ws = getattr(ops, self._KIND.capitalize() + "Workspace")(self._whole, dev) \
            if dev.type == "cuda" else None
        return dev

    def _make_plan(self, plan, t0, nt):
        return self._new_plan(plan, t0, nt).to(self.flat.data.device)

    def _state(self, t0, nt):
        """The views of the ``_LAYOUT`` tensors that belong to tensors ``t0 .. t0 + nt``."""
        w = self._whole
        return tuple(getattr(self, name)[per * getattr(w, offsets)[t0]:
                                         per * getattr(w, offsets)[t0 + nt]]
                     for name, offsets, per in self._LAYOUT)

    def _operands(self, start, length, t0, nt):
        """The state a step of the range takes, in the order of the kernels' and the oracle's
        arguments."""
        return self._state(t0, nt)

    def step_range(self, start, length, grad, grad_scale=1.0):
        t0, nt = self._range(start, length)
        p = self.flat.data[start:start + length]
        state, hp = self._operands(start, length, t0, nt), self._hp()
        if p.is_cuda:
            getattr(ops, self._KIND + "_step")(
                self._plan(start, length), self._ws, p, grad, *state, t=self.steps + 1,
                grad_scale=grad_scale, step=self.step_t, lr_tensor=self.lr_t,
                shadow=self._shadow(start, length), **hp)
            return
        getattr(oracle, self._KIND + "_apply")(
            p, *state, grad.to(torch.float32) * grad_scale, self._tensors(start, length),
            step=self.steps + 1, **{k: getattr(self, k) for k in self._ORACLE_ONLY}, **hp)


class FlatAdafactor(_Factored):
    """Adafactor (Shazeer and Stern, ICML 2018) with an external learning rate
    (``compress/oracle.py adafactor_apply``).  A tensor with ``dim() >= 2``, viewed as ``[n, m] =
    [shape[0], numel / shape[0]]`` like :class:`FlatMuon`'s, keeps ``n + m`` floats of
    second-moment statistics in the flat ``row`` / ``col``; a vector keeps its full second moment
    in ``v``; ``m`` (indexed like ``flat.data``) exists only when ``beta1 > 0``.  ``beta2_t = 1 -
    t^-decay``; the update is clipped to an RMS of ``clip`` per tensor and, with
    ``scale_parameter``, scaled by ``max(1e-3, RMS(p))``.  A step covers one bucket or the whole
    model: four HIP launches on the GPU (``ops.adafactor_step``, which reads ``t`` from the
    device counter ``step_t``), the torch oracle on the CPU."""
    _KIND = "adafactor"
    _STATE = ("row", "col", "v", "m")
    _LAYOUT = (("row", "r0", 1), ("col", "c0", 1), ("v", "v0", 1))
    _COVERS = ("an Adafactor", "statistics are")

    def __init__(self, flat, lr=1e-3, beta1=0.0, clip=1.0, scale_parameter=False,
                 weight_decay=0.0, decay=0.8):
        if not 0.0 <= beta1 < 1.0 or not clip > 0 or not decay > 0:
            raise ValueError(f"Adafactor needs beta1 in [0, 1), clip > 0 and decay > 0, not "
                             f"{beta1!r}, {clip!r}, {decay!r}")
        self.beta1, self.clip, self.decay = float(beta1), float(clip), float(decay)
        self.scale_parameter, self.weight_decay = bool(scale_parameter), weight_decay
        self._init(flat, lr)
        self.m = torch.zeros_like(flat.data) if self.beta1 > 0 else None

    def _new_plan(self, plan, t0, nt):
        return ops.AdafactorPlan(plan, self.rows[t0:t0 + nt])

    def _operands(self, start, length, t0, nt):
        m = self.m[start:start + length] if self.m is not None else None
        return self._state(t0, nt) + (m,)

    def _hp(self):
        return dict(lr=self.lr, beta1=self.beta1, clip=self.clip, decay=self.decay,
                    scale_parameter=self.scale_parameter, weight_decay=self.weight_decay)

    def _tensors(self, start, length):
        """The oracle's ``(offset, numel, rows, s0, s1)`` rows of a range, the state offsets
        counted from the range's views."""
        t0, nt = self._range(start, length)
        w = self._whole
        return [(self.flat.offsets[t] - start, self.flat.params[t].numel(), self.rows[t],
                 (w.r0[t] - w.r0[t0]) if self.rows[t] else (w.v0[t] - w.v0[t0]),
                 w.c0[t] - w.c0[t0]) for t in range(t0, t0 + nt)]


class FlatGalore(_Factored):
    """GaLore (Zhao et al., ICML 2024): Adam whose two moments live in a rank-``rank`` subspace
    of each weight matrix (``compress/oracle.py galore_apply``).  A tensor with ``dim() >= 2``,
    viewed as ``[n, m] = [shape[0], numel / shape[0]]`` like :class:`FlatMuon`'s, whose short side
    ``s`` exceeds ``rank`` keeps a projector ``[s, rank]`` in the flat ``proj`` and the moments of
    its projected gradient (``rank`` times the long side) in ``m_lr`` / ``v_lr``; every other
    tensor keeps full moments in ``m`` / ``v``.  Every ``update_gap`` steps the projector is
    refreshed from the gradient by two rounds of subspace iteration, warm-started from itself;
    the first one is a Gaussian drawn on the CPU from ``seed``.  The projected update is scaled by
    ``scale``.  The weight decay is decoupled (``p (1 - lr wd)``, as Muon's and Lion's), unlike
    :class:`FlatAdam`'s L2 term.  A step covers one bucket or the whole model: a fixed number of
    HIP launches on the GPU (``ops.galore_step``, which reads ``t`` from the device counter
    ``step_t``), the torch oracle on the CPU."""
    kind = _KIND = "galore"
    ITERS = 2
    _STATE = ("proj", "m_lr", "v_lr", "m", "v")
    _LAYOUT = (("proj", "p0", 1), ("m_lr", "l0", 1), ("v_lr", "l0", 1), ("m", "d0", 1),
               ("v", "d0", 1))
    _ORACLE_ONLY = ("rank",)
    _COVERS = ("a GaLore", "projectors are")

    def __init__(self, flat, lr=1e-3, rank=64, update_gap=200, scale=0.25, betas=(0.9, 0.999),
                 eps=1e-8, weight_decay=0.0, seed=0):
        if rank % 16 or not 16 <= rank <= 128 or update_gap < 1 or not scale > 0:
            raise ValueError(f"GaLore needs a rank that is a multiple of 16 in 16..128, "
                             f"update_gap >= 1 and scale > 0, not {rank!r}, {update_gap!r}, "
                             f"{scale!r}")
        self.rank, self.update_gap, self.scale = int(rank), int(update_gap), float(scale)
        self.betas, self.eps, self.weight_decay = tuple(betas), eps, weight_decay
        dev = self._init(flat, lr)
        gen = torch.Generator().manual_seed(seed)
        self.proj = torch.randn(self._whole.p0[-1], generator=gen).to(dev)

    def _new_plan(self, plan, t0, nt):
        return ops.GalorePlan(plan, self.rows[t0:t0 + nt], self.rank)

    def _hp(self):
        return dict(lr=self.lr, update_gap=self.update_gap, scale=self.scale, betas=self.betas,
                    eps=self.eps, weight_decay=self.weight_decay, iters=self.ITERS)

    def _tensors(self, start, length):
        """The oracle's ``(offset, numel, rows, p0, s0)`` rows of a range, the state offsets
        counted from the range's views."""
        t0, nt = self._range(start, length)
        w = self._whole
        return [(self.flat.offsets[t] - start, self.flat.params[t].numel(),
                 self.rows[t] if w.projected[t] else 0, w.p0[t] - w.p0[t0],
                 (w.l0[t] - w.l0[t0]) if w.projected[t] else (w.d0[t] - w.d0[t0]))
                for t in range(t0, t0 + nt)]


class FlatApollo(_Factored):
    """APOLLO (Zhu et al., MLSys 2025): the Adam moments of a rank-``rank`` random projection of
    each weight matrix's gradient, kept only to estimate a learning-rate scale per long-side
    column (``scale_type="channel"``) or per tensor (``"tensor"``; with ``rank=1`` the paper's
    APOLLO-Mini), which multiplies the full-rank raw gradient (``compress/oracle.py
    apollo_apply``).  The tensors are :class:`FlatGalore`'s: a matrix whose short side exceeds
    ``rank`` keeps ``rank`` times its long side in ``m_lr`` / ``v_lr`` and a pair of update norms
    for the norm-growth limiter; every other tensor keeps full moments in ``m`` / ``v``.  The
    projection is +-1 / sqrt(rank) with signs hashed from (``seed``, the tensor's index, the
    epoch ``(t - 1) // update_gap``): it is never stored and never refreshed by a launch.  The
    weight decay is decoupled.  A step covers one bucket or the whole model: three HIP launches on
    the GPU (``ops.apollo_step``, which reads ``t`` from the device counter ``step_t``), the torch
    oracle on the CPU."""
    kind = _KIND = "apollo"
    _STATE = ("m_lr", "v_lr", "m", "v", "norms")
    _HPARAMS = ("seed",)
    # norms: [matrix][parity of the step]
    _LAYOUT = (("m_lr", "l0", 1), ("v_lr", "l0", 1), ("m", "d0", 1), ("v", "d0", 1),
               ("norms", "k0", 2))
    _ORACLE_ONLY = ("rank",)
    _COVERS = ("an APOLLO", "scales and norms are")

    def __init__(self, flat, lr=1e-3, rank=64, update_gap=200, scale=1.0, scale_type="channel",
                 betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0, seed=0):
        if ((rank != 1 and (rank % 16 or not 16 <= rank <= 128)) or update_gap < 1
                or not scale > 0 or scale_type not in ops.APOLLO_SCALE_TYPES):
            raise ValueError(f"APOLLO needs a rank of 1 or a multiple of 16 in 16..128, "
                             f"update_gap >= 1, scale > 0 and a scale type of channel or tensor, "
                             f"not {rank!r}, {update_gap!r}, {scale!r}, {scale_type!r}")
        self.rank, self.update_gap, self.scale = int(rank), int(update_gap), float(scale)
        self.scale_type, self.seed = scale_type, int(seed)
        self.betas, self.eps, self.weight_decay = tuple(betas), eps, weight_decay
        self._init(flat, lr)

    def _new_plan(self, plan, t0, nt):
        return ops.ApolloPlan(plan, self.rows[t0:t0 + nt], self.rank, t0)

    def _hp(self):
        return dict(lr=self.lr, update_gap=self.update_gap, scale=self.scale,
                    scale_type=self.scale_type, betas=self.betas, eps=self.eps,
                    weight_decay=self.weight_decay, seed=self.seed)

    def _tensors(self, start, length):
        """The oracle's ``(offset, numel, rows, gidx, s0, k)`` rows of a range, the state offsets
        counted from the range's views."""
        t0, nt = self._range(start, length)
        w = self._whole
        return [(self.flat.offsets[t] - start, self.flat.params[t].numel(),
                 self.rows[t] if w.projected[t] else 0, t,
                 (w.l0[t] - w.l0[t0]) if w.projected[t] else (w.d0[t] - w.d0[t0]),
                 w.k0[t] - w.k0[t0]) for t in range(t0, t0 + nt)]


def make_optimizer(name, flat, **kw):
    """The optimizer ``optim/kinds.py`` lists under ``name`` (any letter case), built from the
    keywords it takes: the common ones under their own names and its options under theirs
    (``galore_rank=``, ``ns_steps=``, ...).  A keyword it does not take is ignored, and one that
    is ``None`` means the default."""
    from .kinds import KINDS  # the table names the classes above

    name = name.lower()
    if name not in KINDS:
        raise ValueError(f"unknown optimizer {name!r}")
    return KINDS[name].build(flat, kw)
