"""PowerSGD low-rank gradient exchange (``--compress powersgd``; Vogels et al., NeurIPS 2019, what
PyTorch ships as DDP's ``powerSGD_hook``).

Per step and compressed tensor, with M = (gradient + residual) viewed as ``[n, m]``:

1. ``P = M Q`` (Q is ``[m, r]``, warm-started from the previous step);
2. all-reduce P, divide by N, orthogonalise its columns (modified Gram-Schmidt);
3. ``Q = M^T P``; all-reduce Q, divide by N;
4. ``g^ = P Q^T``, ``residual = M - g^``, and every rank takes the same optimizer step with g^
   (momentum on the receiver, after decompression, as in the paper).  Q is kept.

Tensors that are not worth compressing (``compress/plan.py LowRankPlan``: biases, BatchNorm
scales, small matrices) travel whole behind the P factors, in the same all-reduce, and keep no
residual.

Byte model.  The payload is *linear*: small dense fp32 factors averaged by plain all-reduces, with
no re-quantisation.  A bucket's payload is ``4 (p_floats + q_floats)`` bytes and a ring all-reduce
moves ``2 (N - 1) / N`` times that per rank and direction whatever N is -- the all-gather
exchanges receive ``(N - 1)`` payloads -- and the decode does not depend on N at all.

Every bucket costs four codec launches and two collectives per step.  Phases and split graphs
follow ``TwoStageSignExchange``: graph A = forward, backward and the project launches; eager
all-reduce P, orthogonalise, back-project, all-reduce Q; graph B = reconstruct + step.

State: ``resid`` (per rank, ``flat.numel`` floats) and ``q`` (the same on every rank; initial Q
from the counter RNG keyed by (seed, bucket, tensor), mapped to [-1, 1) and orthogonalised once).

Known behaviour, shared with torch's hook: a tensor whose gradient is exactly zero on every rank
drives its Q to zero; it then stays at g^ = 0 while its residual accumulates what arrives later.
Dead columns are not re-seeded.
"""
import torch

from ..compress import oracle
from ..compress.plan import LowRankPlan
from .engine import StepStats, clip_final_grads


def _align(n, a=64):
    return (n + a - 1) // a * a


class PowerSGDExchange:
    def __init__(self, flat, comm, codec, optimizer, clipper=None):
        if codec.kind != "powersgd":
            raise ValueError("the PowerSGD exchange needs --compress powersgd")
        if not flat.attach_grads:
            raise ValueError("the PowerSGD exchange reads the flat gradient buffer")
        if getattr(optimizer, "onebit", False):
            raise ValueError("1-bit Adam runs its own sign exchange, not PowerSGD")
        self.flat, self.comm, self.codec, self.opt = flat, comm, codec, optimizer
        self.device = flat.data.device
        self.N, self.rank = comm.world, comm.rank
        self.inv_n = 1.0 / self.N
        self.nb = len(flat.buckets)
        self.clipper = clipper  # --clip-grad-norm: runs once per step, ahead of the projects
        self.step_idx = 0
        self.lr_plans = [LowRankPlan(b.plan, [tuple(p.shape) for p in b.params], codec.rank)
                         for b in flat.buckets]
        codec.bind_powersgd(self.lr_plans, self.device)
        # one P and two Q buffers for all buckets; bucket bi's slices start 64-float aligned
        self.poff, self.qoff, np_, nq = [], [], 0, 0
        for t in self.lr_plans:
            self.poff.append(np_)
            self.qoff.append(nq)
            np_ += _align(max(t.p_floats, 1))
            nq += _align(max(t.q_floats, 1))
        z = dict(dtype=torch.float32, device=self.device)
        self.p = torch.zeros(np_, **z)
        self.qsum = torch.zeros(nq, **z)  # this step's M^T P, summed by the all-reduce
        self.q = torch.zeros(nq, **z)  # the warm start: last step's averaged Q
        for bi, t in enumerate(self.lr_plans):
            self.q_view(bi)[:t.q_floats].copy_(oracle.powersgd_init_q(t, codec.seed, bi))
        self.resid = torch.zeros_like(flat.grad)
        self.last = StepStats()
        # split-graph protocol (runtime/trainer.py, as ShardedPSExchange's)
        self.use_dev_key = self.dev_key_advance = self.defer_comm = self._active = False
        self.side = None
        self._projected = False
        self.clock = None  # Stopwatch of --phase-timing

    def _mark(self, name):
        if self.clock is not None:
            self.clock.mark(name)

    def p_view(self, bi: int) -> torch.Tensor:
        return self.p[self.poff[bi]:self.poff[bi] + _align(max(self.lr_plans[bi].p_floats, 1))]

    def q_view(self, bi: int, summed: bool = False) -> torch.Tensor:
        buf = self.qsum if summed else self.q
        return buf[self.qoff[bi]:self.qoff[bi] + _align(max(self.lr_plans[bi].q_floats, 1))]

    def begin(self):
        self._projected = False

    def set_device_key(self, step: int = None):
        pass  # no random numbers after the initial Q

    def launch_pending(self):
        """Phase 1: M = g + residual and P = M Q, one launch per bucket."""
        if self._projected:
            return
        self._mark("backward")
        clip_final_grads(self.clipper, self.device)
        for b in self.flat.buckets:
            bi = b.index
            self.codec.ps_project(bi, self.flat.grad_view(b),
                                  self.resid[b.start:b.start + b.length], self.q_view(bi),
                                  self.p_view(bi))
        self._projected = True
        self._mark("encode")

    def join_side(self):
        pass

    def wait(self):
        pass

    def communicate(self):
        """Phase 2: all-reduce P (with the dense tail), orthogonalise, back-project, all-reduce
        Q.  The averaging (1/N) happens in the orthogonalise and reconstruct launches."""
        for b in self.flat.buckets:
            bi, t = b.index, self.lr_plans[b.index]
            rs = self.resid[b.start:b.start + b.length]
            self.comm.all_reduce(self.p_view(bi)[:t.p_floats])
            self._mark("collective")
            self.codec.ps_orthogonalize(bi, self.p_view(bi), self.inv_n)
            self.codec.ps_backproject(bi, rs, self.p_view(bi), self.q_view(bi, True))
            self._mark("aggregate")
            if t.q_floats:
                self.comm.all_reduce(self.q_view(bi, True)[:t.q_floats])
            self._mark("collective")

    def apply(self):
        """Phase 3: reconstruct, residual and optimizer step, one launch per bucket (an optimizer
        without a fused step gets g^ in the flat gradient first)."""
        opt = self.opt
        for b in self.flat.buckets:
            bi, sl = b.index, slice(b.start, b.start + b.length)
            args = (bi, self.resid[sl], self.p_view(bi), self.q_view(bi, True), self.q_view(bi),
                    self.inv_n)
            if getattr(opt, "fusable", False):
                self.codec.ps_decode_apply_sgd(*args, self.flat.data_view(b), opt.mom[sl],
                                               opt.hparams(), opt.first,
                                               shadow=self.flat.shadow_view(b))
            else:
                gv = self.flat.grad_view(b)
                self.codec.ps_decode_apply_sgd(*args, None, None, None, False, grad_out=gv)
                opt.step_range(b.start, b.length, gv, 1.0)
        opt.end_step()

    def finish(self):
        self.launch_pending()
        self.communicate()
        self.apply()
        self._mark("decode_update")
        self._projected = False
        self.last = self.bytes_per_step()
        self.step_idx += 1

    def bytes_per_step(self):
        s = StepStats()
        for b, t in zip(self.flat.buckets, self.lr_plans):
            payload = 4 * (t.p_floats + t.q_floats)
            s.payload_bytes += payload
            s.dense_bytes += b.plan.numel * 4
            wire = 2 * (self.N - 1) * payload // self.N  # two ring all-reduces
            s.wire_bytes_sent += wire
            s.wire_bytes_recv += wire
            s.collectives += 2 if t.q_floats else 1
        return s

    def close(self):
        pass
