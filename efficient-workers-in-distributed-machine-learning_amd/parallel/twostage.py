"""Two-stage sign all-reduce with worker and server error feedback (``--topology twostage``).

1-bit Adam's communication scheme (Tang et al., ICML 2021; DeepSpeed ``compressed_allreduce``), for
the sign codec under SGD and under 1-bit Adam's compressed stage:

1. every rank sign-compresses its gradient (1-bit Adam: its momentum candidate) with its *worker*
   residual, shard by shard (``shard_plans``: N contiguous chunk-aligned shards per bucket);
2. one ``all_to_all`` hands shard r of every rank's payload to rank r;
3. rank r averages the N payloads of its shard, adds its *server* residual and sign-compresses
   again (``Codec.ts_reduce_encode``: one kernel, no dense scratch);
4. one ``all_gather`` of the N re-compressed shards; every rank decodes them and takes the same
   optimizer step, so the replicas stay identical.

Byte model.  With D gradient elements a bucket's payload is about D/8 bytes and a shard's P is
about D/(8 N).  Each collective moves (N - 1) P bytes per rank and direction, so a step sends and
receives 2 (N - 1) P = 2 (N - 1)/N * D/8 bytes whatever N is; the all-gather exchange
(``engine.py``) receives (N - 1) D/8.  Two-stage receives less for every N >= 3 and the same at
N = 2 (2 * 1/2 = 1), at the price of a second quantisation and a second collective.  Both
quantisations are error-compensated.

Every bucket costs exactly three codec launches per step whatever N is: the push encode and the
pull decode address the ``[N, P]`` row buffers through a per-chunk slot table
(``compress/plan.py TwoStagePlan``), the owner step is one fused kernel.  A rank whose shard of a
bucket is empty (fewer chunks than ranks) launches no owner step for it and sends a zero row.

Per-rank state: ``resid`` (worker residual, ``flat.numel`` elements) and ``sresid`` (server
residual: one slot per bucket sized to that bucket's largest shard, so every rank's tensor has the
same length and a checkpoint can all-gather the rows).

``TwoStageVoteExchange`` below is the same scheme for Distributed Lion's vote (``--compress vote
--vote-exchange twostage``): integer counting instead of averaging, no scales and no residuals.
"""
import torch

from ..compress.plan import TwoStagePlan
from .engine import StepStats, clip_final_grads
from .sharded import shard_plans


def _align(n, a=64):
    return (n + a - 1) // a * a


class TwoStageSignExchange:
    """All ranks are workers and each owns one shard of every bucket (see module docstring).
    Follows ``ShardedPSExchange``'s phases and its split-graph protocol: graph A = forward,
    backward and the push encodes; eager all-to-all, owner kernel and all-gather; graph B = the
    pull decode + optimizer step."""

    def __init__(self, flat, comm, codec, optimizer, clipper=None):
        if codec.kind != "sign":
            raise ValueError("--topology twostage is the sign codec's exchange: it needs "
                             "--compress sign")
        if not flat.attach_grads:
            raise ValueError("the two-stage exchange reads the flat gradient buffer")
        self.flat, self.comm, self.codec, self.opt = flat, comm, codec, optimizer
        self.device = flat.data.device
        self.N, self.rank = comm.world, comm.rank
        self.nb = len(flat.buckets)
        self.onebit = bool(getattr(optimizer, "onebit", False))
        self.clipper = clipper  # --clip-grad-norm: runs once per step, ahead of the push encodes
        self.step_idx = 0
        self.ts = [TwoStagePlan(b.plan, shard_plans(b.plan, self.N, b.start))
                   for b in flat.buckets]
        codec.bind_twostage(self.ts, self.device)
        z = dict(dtype=torch.uint8, device=self.device)
        # rows are zero at allocation; the kernels write scales and words only, and an empty
        # shard's row is never written at all
        self.send = [torch.zeros((self.N, t.P), **z) for t in self.ts]
        self.recv = [torch.zeros((self.N, t.P), **z) for t in self.ts]
        self.gathered = [torch.zeros((self.N, t.P), **z) for t in self.ts]
        self.own = [g[self.rank] for g in self.gathered]
        self.resid = torch.zeros_like(flat.grad)  # worker residual
        self.soff, n = [], 0
        for t in self.ts:  # server residual: bucket bi's slot is sresid[soff[bi]:][:max_shard]
            self.soff.append(n)
            n += _align(t.max_shard)
        self.sresid = torch.zeros(n, dtype=torch.float32, device=self.device)
        self.last = StepStats()
        # split-graph protocol (runtime/trainer.py, as ShardedPSExchange's)
        self.use_dev_key = self.dev_key_advance = self.defer_comm = self._active = False
        self.key_state = torch.zeros(2, dtype=torch.int32, device=self.device)
        self.key_dev = self.key_state[1:2]
        self.side = None
        self._encoded = False
        self.clock = None  # Stopwatch of --phase-timing

    def _mark(self, name):
        if self.clock is not None:
            self.clock.mark(name)

    def begin(self):
        self._encoded = False

    def set_device_key(self, step: int = None):
        pass  # the sign codec draws no random numbers

    def sresid_view(self, bi: int) -> torch.Tensor:
        """Bucket ``bi``'s slot of the server residual (relative to this rank's shard start)."""
        return self.sresid[self.soff[bi]:self.soff[bi] + _align(self.ts[bi].max_shard)]

    def launch_pending(self):
        """Phase 1: the push encode, one launch per bucket over all N shards."""
        if self._encoded:
            return
        self._mark("backward")
        clip_final_grads(self.clipper, self.device)
        o = self.opt
        for b in self.flat.buckets:
            sl = slice(b.start, b.start + b.length)
            mom = None
            if self.onebit:  # sign(exp_avg * beta1 + (1 - beta1) * (g + wd * p) + residual)
                mom = dict(exp_avg=o.exp_avg[sl], beta1=o.betas[0], weight_decay=o.weight_decay,
                           param=self.flat.data_view(b))
            self.codec.ts_encode(b.index, self.flat.grad_view(b), self.send[b.index],
                                 self.resid[sl], mom)
        self._encoded = True
        self._mark("encode")

    def join_side(self):
        pass

    def wait(self):
        pass

    def communicate(self):
        """Phase 2: all-to-all of the shard rows, the owner's average + re-encode (one launch),
        all-gather of the owners' rows."""
        for b in self.flat.buckets:
            bi = b.index
            self.comm.all_to_all(self.recv[bi], self.send[bi])
            self._mark("collective")
            if self.ts[bi].shards[self.rank][2] is not None:
                self.codec.ts_reduce_encode(bi, self.rank, self.recv[bi], self.own[bi],
                                            1.0 / self.N, self.sresid_view(bi))
            self._mark("aggregate")
            self.comm.all_gather(self.gathered[bi].view(-1), self.own[bi])
            self._mark("collective")

    def apply(self):
        """Phase 3: the pull decode of all N shards fused with the optimizer step, one launch per
        bucket (an optimizer without a fused step decodes into the flat gradient first)."""
        opt = self.opt
        for b in self.flat.buckets:
            bi, sl = b.index, slice(b.start, b.start + b.length)
            if self.onebit:
                self.codec.ts_decode_apply_onebit(bi, self.gathered[bi], self.flat.data_view(b),
                                                  opt.exp_avg[sl], opt.exp_avg_sq[sl],
                                                  opt.hparams(), shadow=self.flat.shadow_view(b),
                                                  rank=self.rank)
            elif getattr(opt, "fusable", False):
                self.codec.ts_decode_apply_sgd(bi, self.gathered[bi], self.flat.data_view(b),
                                               opt.mom[sl], opt.hparams(), opt.first,
                                               shadow=self.flat.shadow_view(b), rank=self.rank)
            else:
                gv = self.flat.grad_view(b)
                self.codec.ts_decode_apply_sgd(bi, self.gathered[bi], None, None, None, False,
                                               grad_out=gv)
                opt.step_range(b.start, b.length, gv, 1.0)
        opt.end_step()

    def finish(self):
        self.launch_pending()
        self.communicate()
        self.apply()
        self._mark("decode_update")
        self._encoded = False
        self.last = self.bytes_per_step()
        self.step_idx += 1

    def bytes_per_step(self):
        s = StepStats()
        for b, t in zip(self.flat.buckets, self.ts):
            s.payload_bytes += sum(lay.nbytes for _, _, _, lay, _ in t.shards if lay is not None)
            s.dense_bytes += b.plan.numel * 4
            s.wire_bytes_sent += 2 * (self.N - 1) * t.P  # all-to-all rows + ring all-gather
            s.wire_bytes_recv += 2 * (self.N - 1) * t.P
            s.collectives += 2
        return s

    def close(self):
        pass


class TwoStageVoteExchange:
    """Distributed Lion's vote as workers -> owner -> workers, one bit per element in each
    direction (``--compress vote --vote-exchange twostage``; Liu et al. 2024).

    For each bucket, cut into N chunk-aligned shards by ``shard_plans``:

    1. push: every rank votes as the all-gather exchange does (``encode_vote``: the sign of its own
       Lion direction, an exact zero by the parity of index + step + rank; its momentum then moves
       with beta2), shard r's bits into row r of an ``[N, P]`` buffer;
    2. one ``all_to_all``: rank r receives the N votes on its shard;
    3. owner step (``Codec.ts_vote_reduce``): ``s = N - 2 * set`` per element, the bit sent back is
       ``(s < 0) | (s == 0 & the owner's own bit)`` -- one bit cannot say 0, so a tie takes the
       owner's vote.  Integer arithmetic only; ties cannot occur at odd N;
    4. one ``all_gather`` of the N owner rows;
    5. pull: every rank steps by ``d = 1 - 2 * bit`` of each shard's row, so the replicas agree by
       construction.

    At odd N (and N = 1) parameters and momenta are bitwise those of the all-gather ``majority``
    vote; at even N wherever ``s != 0`` (the all-gather vote steps by 0 on a tie, this exchange by
    the owner's sign).  ``average`` is refused: a mean does not fit one bit.

    Byte model.  A shard's row is ``P = 1024 * (its chunks)`` bytes, about D/(8 N).  Each
    collective moves (N - 1) P bytes per rank and direction, so a step sends and receives 2 (N -
    1) P = 2 (N - 1)/N * D/8 bytes whatever N is, where the all-gather vote receives (N - 1) D/8.

    Three codec launches per bucket and step (push, owner, pull); a rank whose shard of a bucket
    is empty launches no owner step for it and sends a zero row.  No residual and no scale: the
    only per-rank state is the optimizer's own ``exp_avg``, which the trainer checkpoints as
    ``lion_momentum [world, numel]`` (``vote = True``).  The push reads the flat gradient buffer,
    as the sign exchange does; a pointer-mode encode is out of scope.  Follows
    ``TwoStageSignExchange``'s phases and split-graph protocol: graph A = forward, backward, clip
    and the push encodes; eager all-to-all, owner kernel and all-gather; graph B = the apply."""

    vote = True

    def __init__(self, flat, comm, codec, optimizer, clipper=None):
        if codec.kind != "vote" or codec.aggregate != "majority":
            raise ValueError("--vote-exchange twostage is the vote codec's exchange with the "
                             "majority aggregate: a mean does not fit the one bit sent back")
        if not getattr(optimizer, "lion", False):
            raise ValueError("the vote codec's payload carries no magnitudes: only Lion "
                             "(--optimizer lion) can step on it")
        if not flat.attach_grads:
            raise ValueError("the two-stage exchange reads the flat gradient buffer")
        self.flat, self.comm, self.codec, self.opt = flat, comm, codec, optimizer
        self.device = flat.data.device
        self.N, self.rank = comm.world, comm.rank
        self.nb = len(flat.buckets)
        self.clipper = clipper  # --clip-grad-norm: runs once per step, ahead of the push encodes
        self.step_idx = 0
        self.ts = [TwoStagePlan(b.plan, shard_plans(b.plan, self.N, b.start), kind="vote")
                   for b in flat.buckets]
        codec.bind_twostage(self.ts, self.device)
        z = dict(dtype=torch.uint8, device=self.device)
        # rows are zero at allocation; the kernels write words only, and an empty shard's row is
        # never written at all
        self.send = [torch.zeros((self.N, t.P), **z) for t in self.ts]
        self.recv = [torch.zeros((self.N, t.P), **z) for t in self.ts]
        self.gathered = [torch.zeros((self.N, t.P), **z) for t in self.ts]
        self.own = [g[self.rank] for g in self.gathered]
        self.last = StepStats()
        # split-graph protocol (runtime/trainer.py, as TwoStageSignExchange's)
        self.use_dev_key = self.dev_key_advance = self.defer_comm = self._active = False
        self.key_state = torch.zeros(2, dtype=torch.int32, device=self.device)
        self.key_dev = self.key_state[1:2]
        self.side = None
        self._encoded = False
        self.clock = None  # Stopwatch of --phase-timing

    def _mark(self, name):
        if self.clock is not None:
            self.clock.mark(name)

    def begin(self):
        self._encoded = False

    def set_device_key(self, step: int = None):
        pass  # the vote draws no random numbers (the dither reads the optimizer's step counter)

    def launch_pending(self):
        """Phase 1: the push encode, one launch per bucket over all N shards."""
        if self._encoded:
            return
        self._mark("backward")
        clip_final_grads(self.clipper, self.device)
        o = self.opt
        for b in self.flat.buckets:
            self.codec.ts_encode_vote(b.index, self.flat.grad_view(b), self.send[b.index],
                                      o.exp_avg[b.start:b.start + b.length], o.betas,
                                      o.steps + 1, self.rank, step_tensor=o.step_t)
        self._encoded = True
        self._mark("encode")

    def join_side(self):
        pass

    def wait(self):
        pass

    def communicate(self):
        """Phase 2: all-to-all of the shard rows, the owner's count (one launch), all-gather of
        the owners' rows."""
        for b in self.flat.buckets:
            bi = b.index
            self.comm.all_to_all(self.recv[bi], self.send[bi])
            self._mark("collective")
            if self.ts[bi].shards[self.rank][2] is not None:
                self.codec.ts_vote_reduce(bi, self.rank, self.recv[bi], self.own[bi])
            self._mark("aggregate")
            self.comm.all_gather(self.gathered[bi].view(-1), self.own[bi])
            self._mark("collective")

    def apply(self):
        """Phase 3: Lion's step by the owners' bits, one launch per bucket; the last bucket's
        launch advances the device RNG key of a captured step."""
        opt = self.opt
        for b in self.flat.buckets:
            adv = self.dev_key_advance and self.use_dev_key and b.index == self.nb - 1
            self.codec.ts_decode_apply_vote(b.index, self.gathered[b.index],
                                            self.flat.data_view(b), opt.hparams(),
                                            shadow=self.flat.shadow_view(b),
                                            key_state=self.key_state if adv else None,
                                            rank=self.rank)
        opt.end_step()

    def finish(self):
        self.launch_pending()
        self.communicate()
        self.apply()
        self._mark("decode_update")
        self._encoded = False
        self.last = self.bytes_per_step()
        self.step_idx += 1

    def bytes_per_step(self):
        s = StepStats()
        for b, t in zip(self.flat.buckets, self.ts):
            s.payload_bytes += sum(lay.nbytes for _, _, _, lay, _ in t.shards if lay is not None)
            s.dense_bytes += b.plan.numel * 4
            s.wire_bytes_sent += 2 * (self.N - 1) * t.P  # all-to-all rows + ring all-gather
            s.wire_bytes_recv += 2 * (self.N - 1) * t.P
            s.collectives += 2
        return s

    def close(self):
        pass
