"""Count-sketch gradient exchange (``--compress sketch``; SketchedSGD: Ivkin, Rothchild, Ullah,
Braverman, Stoica, Arora, "Communication-efficient Distributed SGD with Sketching", NeurIPS 2019).

The sparsifying codecs of the all-gather exchange apply the union of every rank's local top-k.  A
count sketch is linear, so the ranks' sketches are summed by a plain all-reduce and what is
recovered are the heavy coordinates of the *summed* gradient.  Per step and bucket, with the
bucket's top-k plan (k per tensor) and its ``SketchPlan`` (``compress/plan.py``):

1. ``acc = g + residual`` on the sketched tensors, kept in the residual;
2. the table ``T[R][W]`` of ``acc``; all-reduce T (sum);
3. ``est[i]`` = the median over the rows of the signed table entries of ``i``;
4. per tensor the project's top-k of ``est`` -- the same set on every rank, because T is;
5. ``vals`` = this rank's own ``acc`` at the selected coordinates, which leave the residual;
   all-reduce ``vals`` (sum);
6. ``g^ = vals / N`` at the selected coordinates, 0 elsewhere, and every rank takes the same
   optimizer step (momentum on the receiver, after the exchange).

Tensors with ``k == numel`` (``--topk-dense-below``, ratio 1) are *dense*: not sketched, always
selected whole, no residual; their gradients ride in the second all-reduce.

Byte model.  A bucket's payload is ``4 (R W + K + dense elements)`` bytes (K = the sum of k over
its sketched tensors) and each of the two ring all-reduces moves ``2 (N - 1) / N`` times its part
per rank and direction whatever N is; the decode does not depend on N.  The all-gather ``topk``
receives ``(N - 1)`` payloads of about ``6 K`` bytes.

Phases and split graphs follow ``PowerSGDExchange``: graph A = forward, backward, stage and table;
eager all-reduce T, estimate, select, gather, all-reduce vals; graph B = decode + step.

State: ``resid`` (per rank, ``flat.numel`` floats).  The hashes are functions of (seed, bucket)
alone, the same on every rank and step: the sketch is linear across ranks and a captured graph
takes no new input.
"""
import torch

from .engine import StepStats, clip_final_grads


def _align(n, a=64):
    return (n + a - 1) // a * a


class SketchExchange:
    def __init__(self, flat, comm, codec, optimizer, clipper=None):
        if codec.kind != "sketch":
            raise ValueError("the sketch exchange needs --compress sketch")
        if not flat.attach_grads:
            raise ValueError("the sketch exchange reads the flat gradient buffer")
        if getattr(optimizer, "onebit", False):
            raise ValueError("1-bit Adam runs its own sign exchange, not the sketch")
        self.flat, self.comm, self.codec, self.opt = flat, comm, codec, optimizer
        self.device = flat.data.device
        self.N, self.rank = comm.world, comm.rank
        self.inv_n = 1.0 / self.N
        self.nb = len(flat.buckets)
        self.clipper = clipper  # --clip-grad-norm: runs once per step, ahead of the stage
        self.step_idx = 0
        self.resid = torch.zeros_like(flat.grad)
        # the estimate of every bucket: written on sketched tensors only, 0 elsewhere for good
        self.est = torch.zeros_like(flat.grad)
        self._plan()
        self.last = StepStats()
        # split-graph protocol (runtime/trainer.py, as PowerSGDExchange's)
        self.use_dev_key = self.dev_key_advance = self.defer_comm = self._active = False
        self.side = None
        self._sketched = False
        self.clock = None  # Stopwatch of --phase-timing

    def _plan(self):
        """Bind the codec at its current density and size the table and payload buffers: one
        table buffer for all buckets, bucket bi's slice 64-float aligned."""
        self.codec.bind_sketch([b.plan for b in self.flat.buckets], self.device)
        self.sk = self.codec.sk
        self.toff, n = [], 0
        for t in self.sk:
            self.toff.append(n)
            n += _align(t.table_floats)
        self.table = torch.zeros(n, dtype=torch.float32, device=self.device)
        self.payload = [torch.zeros(lay.nbytes, dtype=torch.uint8, device=self.device)
                        for lay in self.codec.layouts]

    def set_ratio(self, ratio: float):
        """Density warm-up: k per tensor, and with it every W and payload, change (every rank at
        the same step; a captured step graph must be re-captured)."""
        if ratio == self.codec.ratio:
            return False
        self.codec.set_ratio(ratio)
        self._plan()
        return True

    def _mark(self, name):
        if self.clock is not None:
            self.clock.mark(name)

    def table_view(self, bi: int) -> torch.Tensor:
        return self.table[self.toff[bi]:self.toff[bi] + self.sk[bi].table_floats]

    def _views(self, b):
        sl = slice(b.start, b.start + b.length)
        return self.flat.grad_view(b), self.resid[sl], self.est[sl]

    def begin(self):
        self._sketched = False

    def set_device_key(self, step: int = None):
        pass  # no random numbers: the hashes are fixed

    def launch_pending(self):
        """Phase 1: acc = g + residual and its table, two launches per bucket."""
        if self._sketched:
            return
        self._mark("backward")
        clip_final_grads(self.clipper, self.device)
        for b in self.flat.buckets:
            g, rs, _ = self._views(b)
            self.codec.sk_sketch(b.index, g, rs, self.table_view(b.index))
        self._sketched = True
        self._mark("encode")

    def join_side(self):
        pass

    def wait(self):
        pass

    def communicate(self):
        """Phase 2: all-reduce the table, estimate, select and gather, all-reduce the values.
        The averaging (1/N) happens in the decode."""
        for b in self.flat.buckets:
            bi = b.index
            g, rs, est = self._views(b)
            self.comm.all_reduce(self.table_view(bi))
            self._mark("collective")
            self.codec.sk_select_gather(bi, self.table_view(bi), est, g, rs, self.payload[bi])
            self._mark("aggregate")
            self.comm.all_reduce(self.codec.sk_values(bi, self.payload[bi]))
            self._mark("collective")

    def apply(self):
        """Phase 3: decode and optimizer step, one launch per bucket (an optimizer without a
        fused step gets g^ in the flat gradient first)."""
        opt = self.opt
        for b in self.flat.buckets:
            bi, sl = b.index, slice(b.start, b.start + b.length)
            if getattr(opt, "fusable", False):
                self.codec.sk_decode_apply_sgd(bi, self.payload[bi], self.inv_n,
                                               self.flat.data_view(b), opt.mom[sl], opt.hparams(),
                                               opt.first, shadow=self.flat.shadow_view(b))
            else:
                gv = self.flat.grad_view(b)
                self.codec.sk_decode_apply_sgd(bi, self.payload[bi], self.inv_n, None, None, None,
                                               False, grad_out=gv)
                opt.step_range(b.start, b.length, gv, 1.0)
        opt.end_step()

    def finish(self):
        self.launch_pending()
        self.communicate()
        self.apply()
        self._mark("decode_update")
        self._sketched = False
        self.last = self.bytes_per_step()
        self.step_idx += 1

    def bytes_per_step(self):
        s = StepStats()
        for b, t in zip(self.flat.buckets, self.sk):
            payload = 4 * t.payload_floats
            s.payload_bytes += payload
            s.dense_bytes += b.plan.numel * 4
            wire = 2 * (self.N - 1) * payload // self.N  # two ring all-reduces
            s.wire_bytes_sent += wire
            s.wire_bytes_recv += wire
            s.collectives += 2
        return s

    def close(self):
        pass
