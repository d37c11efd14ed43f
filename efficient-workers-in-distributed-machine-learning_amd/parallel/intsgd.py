"""IntSGD gradient exchange (``--compress intsgd``; Mishchenko, Wang, Kovalev, Richtarik, "IntSGD:
Adaptive Floatless Compression of Stochastic Gradients", ICLR 2022).

Every quantising codec of the all-gather exchange receives ``(N - 1)`` payloads and decodes N rows.
Here all ranks multiply their gradient by the same scale ``alpha``, round stochastically to
integers in ``[-q, q]``, ``q = floor(127 / N)``, and one int8 all-reduce per bucket sums the codes
in place: ``N q <= 127``, so no sum leaves the range, and the decode reads one row whatever N is.
Per step and bucket:

1. ``acc = g`` (``g + residual`` with error feedback); ``code = clamp(round_stochastic(acc *
   alpha), -q, q)``; with error feedback ``residual = acc - code / alpha``;
2. all-reduce the int8 codes (sum);
3. ``g^ = sum / (alpha N)`` and every rank takes the same fused SGD step; the same launch writes
   the per-chunk sums of ``(p_new - p_old)^2``.

After the last bucket's step one single-block launch forms the next scale from them
(``oracle.intsgd_alpha``, this project's form of the paper's Algorithm 2): the parameters are
replica-identical bit for bit, so ``alpha`` is too, with no collective.

The first step has no update to measure.  It travels dense, as in the paper: an fp32 all-reduce of
the flat gradient and the optimizer's own step, around which the update norm is taken from a copy of
the parameters.  It always runs eagerly.

Byte model.  A bucket's payload is its padded length L in bytes, and the ring all-reduce moves ``2
(N - 1) L / N`` per rank and direction: D bytes each way at N = 2, as ``qsgd`` at 8 bits, which
receives ``(N - 1) D``.

Phases and split graphs follow ``SketchExchange``: graph A = forward, backward, clip, encode; eager
all-reduce; graph B = decode + step of every bucket and the scale launch.

State: the scale (``codec.int_state``: ``r``, ``alpha`` and its two inverses, the same on every
rank) and, with error feedback, ``resid`` (per rank).
"""
import warnings

import torch

from .engine import StepStats, clip_final_grads, upload_device_key


class IntSGDExchange:
    def __init__(self, flat, comm, codec, optimizer, clipper=None, error_feedback=False):
        if codec.kind != "intsgd":
            raise ValueError("the IntSGD exchange needs --compress intsgd")
        if not flat.attach_grads:
            raise ValueError("the IntSGD exchange reads the flat gradient buffer")
        if not getattr(optimizer, "fusable", False):
            raise ValueError("IntSGD's scale is derived for SGD, where update / lr is a gradient: "
                             "it needs --optimizer sgd")
        self.flat, self.comm, self.codec, self.opt = flat, comm, codec, optimizer
        self.device = flat.data.device
        self.N, self.rank = comm.world, comm.rank
        self.nb = len(flat.buckets)
        self.clipper = clipper  # --clip-grad-norm: runs once per step, ahead of the encode
        self.codec.bind_intsgd([b.plan for b in flat.buckets], self.device, self.N)
        self.payload = [torch.zeros(lay.nbytes, dtype=torch.uint8, device=self.device)
                        for lay in self.codec.layouts]
        self.resid = torch.zeros_like(flat.grad) if error_feedback else None
        self.step_idx = 0
        self.have_scale = False  # False: the next step travels dense and produces the scale
        self._warned = False
        self.last = StepStats()
        # split-graph protocol (runtime/trainer.py, as SketchExchange's); the device RNG key
        # {step, key} as GradientExchange keeps it
        self.use_dev_key = self.dev_key_advance = self.defer_comm = self._active = False
        self.key_state = torch.zeros(2, dtype=torch.int32, device=self.device)
        self.key_dev = self.key_state[1:2]
        self._key_ring, self._key_slot = None, 0
        self.side = None
        self._encoded = False
        self.clock = None  # Stopwatch of --phase-timing

    # -- state -----------------------------------------------------------------------------------
    @property
    def dense_step(self) -> bool:
        """The next step is the dense one (no scale yet): it runs eagerly."""
        return not self.have_scale

    def state(self) -> dict:
        """The scale state for a checkpoint (synchronises)."""
        return self.codec.int_state.values() if self.have_scale else None

    def load_state(self, st):
        """Continue from a checkpoint's scale; None (a checkpoint without one): the next step
        travels dense again, with one warning."""
        if st is None:
            self.have_scale = False
            if not self._warned and self.rank == 0:
                warnings.warn("resume: the checkpoint holds no intsgd_state, IntSGD takes one "
                              "dense step to measure its scale")
            self._warned = True
            return
        self.codec.int_state.load(st)
        self.have_scale = True

    def codec_health(self) -> dict:
        """This rank's scale and the fraction of elements the last encode clipped (synchronises:
        read at log records only).  Nothing before the first scale exists."""
        if not self.have_scale:
            return {}
        return {"intsgd_alpha": self.codec.int_state.values()["alpha"],
                "intsgd_sat_frac": int(self.codec.int_sat.sum()) / max(1, self.codec.int_numel)}

    def _mark(self, name):
        if self.clock is not None:
            self.clock.mark(name)

    # -- step protocol ---------------------------------------------------------------------------
    def begin(self):
        self._encoded = False

    def set_device_key(self, step: int = None):
        """Upload this step's RNG state {step, key} (a captured encode reads the key from device
        memory), as ``GradientExchange.set_device_key``."""
        upload_device_key(self, self.step_idx if step is None else step)

    def launch_pending(self):
        """Phase 1: the clip, then one encode launch per bucket (the dense step encodes nothing)."""
        if self._encoded:
            return
        self._mark("backward")
        clip_final_grads(self.clipper, self.device)
        if self.have_scale:
            for b in self.flat.buckets:
                sl = slice(b.start, b.start + b.length)
                self.codec.int_encode(b.index, self.flat.grad_view(b), self.payload[b.index],
                                      self.step_idx, self.rank,
                                      None if self.resid is None else self.resid[sl],
                                      key_tensor=self.key_dev if self.use_dev_key else None)
        self._encoded = True
        self._mark("encode")

    def join_side(self):
        pass

    def wait(self):
        pass

    def communicate(self):
        """Phase 2: one int8 all-reduce per bucket, summed in place (the dense step: one fp32
        all-reduce of the flat gradient)."""
        if not self.have_scale:
            self.comm.all_reduce(self.flat.grad)
        else:
            for b in self.flat.buckets:
                self.comm.all_reduce(self.payload[b.index].view(torch.int8))
        self._mark("collective")

    def apply(self):
        """Phase 3: decode + step + update-norm partials, one launch per bucket, then the scale."""
        opt = self.opt
        hp = opt.hparams()
        if not self.have_scale:
            prev = self.flat.data.clone()
            for b in self.flat.buckets:
                opt.step_range(b.start, b.length, self.flat.grad_view(b), 1.0 / self.N)
            opt.end_step()
            for b in self.flat.buckets:
                self.codec.int_update_norm(b.index, self.flat.data_view(b),
                                           prev[b.start:b.start + b.length])
            self.codec.int_alpha(hp["lr"], hp.get("lr_t"))
            self.have_scale = True
            return
        for b in self.flat.buckets:
            adv = self.dev_key_advance and self.use_dev_key and b.index == self.nb - 1
            self.codec.int_decode_apply(b.index, self.payload[b.index], self.flat.data_view(b),
                                        opt.mom[b.start:b.start + b.length], hp, opt.first,
                                        shadow=self.flat.shadow_view(b),
                                        key_state=self.key_state if adv else None, rank=self.rank)
        opt.end_step()
        self.codec.int_alpha(hp["lr"], hp.get("lr_t"))

    def finish(self):
        dense = not self.have_scale
        self.launch_pending()
        self.communicate()
        self.apply()
        self._mark("decode_update")
        self._encoded = False
        self.last = self.bytes_per_step(dense)
        self.step_idx += 1

    def bytes_per_step(self, dense: bool = None):
        """One collective per bucket of L bytes; the dense step: one of ``4 numel`` bytes."""
        dense = (not self.have_scale) if dense is None else dense
        s = StepStats()
        N = self.N
        if dense:
            payload = 4 * self.flat.numel
            s.payload_bytes = payload
            s.dense_bytes = sum(b.plan.numel * 4 for b in self.flat.buckets)
            wire = 2 * (N - 1) * payload // N
            s.wire_bytes_sent = s.wire_bytes_recv = wire
            s.collectives = 1
            return s
        for b, lay in zip(self.flat.buckets, self.codec.layouts):
            s.payload_bytes += lay.nbytes
            s.dense_bytes += b.plan.numel * 4
            wire = 2 * (N - 1) * lay.nbytes // N
            s.wire_bytes_sent += wire
            s.wire_bytes_recv += wire
            s.collectives += 1
        return s

    def close(self):
        pass
