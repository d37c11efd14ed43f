"""Gradient codecs: one object per exchange, bound to the bucket plans of a model.

``kind``:
  * ``none``  -- dense fp32 all-reduce (reference Method 3, push+pull of raw gradients)
  * ``fp16`` / ``bf16`` -- dense half-precision all-reduce (Horovod ``Compression.fp16``,
    ``horvod_pytorch.py:191-192``)
  * ``qsgd``  -- dense stochastic quantisation to int8/int4 (Method 4)
  * ``topk``  -- top-k sparsification, fp32 values (``TopKCompressor``)
  * ``topk_qsgd`` -- top-k then QSGD (Method 5); the flagship codec
  * ``sign``  -- scaled sign, 1 bit per element plus one fp32 scale per 8192-element chunk
    (1-bit SGD / EF-signSGD); meant to run with error feedback, which the all-gather exchange keeps.
    ``rotate="hadamard"`` (``codec.rotate``; DRIVE / EDEN): the signs are taken of a randomised
    Hadamard rotation of every chunk, the same payload, one inverse transform on the receiver
  * ``vote``  -- Distributed Lion's 1-bit majority vote (Liu et al. 2024): one bit per element, the
    sign of the rank's own Lion update direction; no scale, no residual (``encode_vote`` /
    ``decode_apply_vote``; needs ``optim/flat.py FlatLion``)
  * ``mx``    -- OCP Microscaling block floating point (``fmt``: ``fp8`` = MXFP8, E4M3 elements;
    ``fp4`` = MXFP4, E2M1): every 32 elements share one power-of-two scale byte; runs with error
    feedback on the all-gather exchange, one encode and one fused decode launch per bucket
  * ``tern``  -- TernGrad (Wen et al. 2017): stochastic ternary codes {-1, 0, +1} at 2 bits per
    element and one fp32 scaler per tensor, ``min(max|g|, clip * rms(g))`` (``clip``, default 2.5;
    0 = no clipping, then unbiased).  ``rms`` is taken about zero, not about the mean, and every
    rank's codes are decoded with that rank's own scaler (no scaler sharing).  Runs on the
    all-gather exchange, error feedback optional (off by default); three encode launches and one
    fused decode launch per bucket
  * ``thresh`` -- threshold-search sparsification (RedSync, Fang et al. 2019; MSTopK, Shi et al.
    2021; hard-threshold sparsification, Sahu et al. 2021): per 8192-element chunk everything at
    or above a canonical bf16-level threshold chosen so that at most the chunk's share of the
    tensor's top-k quota is sent, with the exact fp32 values; no exact selection.  Runs on the
    all-gather exchange with plain error feedback, one encode and one fused decode launch per
    bucket
  * ``powersgd`` -- rank-r factors of the error-compensated gradient matrices (PowerSGD, Vogels et
    al. 2019), averaged by two small fp32 all-reduces (``parallel/powersgd.py``; the ``ps_*``
    methods below)
  * ``sketch`` -- a count sketch of the error-compensated gradient (SketchedSGD, Ivkin et al.
    2019): ``rows`` x W fp32 table summed by one all-reduce, the heavy coordinates of the *sum*
    recovered from it and their exact values summed by a second one (``parallel/sketch.py``; the
    ``sk_*`` methods below); ``ratio`` / ``dense_below`` give k per tensor as for ``topk``
  * ``intsgd`` -- IntSGD (Mishchenko et al. 2022): every rank rounds ``g * alpha`` stochastically
    to int8 codes in ``[-q, q]``, ``q = floor(127 / N)``, with one model-wide ``alpha`` that every
    replica derives from the norm of the last update, and the codes are summed by one int8
    all-reduce per bucket (``parallel/intsgd.py``; the ``int_*`` methods below); error feedback
    optional (off by default)

Device tensors go through the HIP kernels (``ops``); CPU tensors through the torch oracle.  On a
GPU box a missing extension raises instead of silently falling back.
"""
import os

import torch

from .. import ops

# EWDML_ORACLE=1: run the torch oracle on device tensors too (eager experiments with codec
# variants before they have kernels; needs flat gradient views, EWDML_GRAD_VIEWS=1)
_FORCE_ORACLE = os.environ.get("EWDML_ORACLE") == "1"
from . import oracle
from .plan import POWERSGD_RANKS, SKETCH_ROWS, BucketPlan, Layout, SketchPlan
from .rng import stream_key

KINDS = ("none", "fp16", "bf16", "qsgd", "topk", "topk_qsgd", "sign", "powersgd", "vote", "mx",
         "tern", "sketch", "thresh", "intsgd")
VOTE_AGGREGATES = ("majority", "average")
SIGN_ROTATIONS = ("none", "hadamard")
MX_FORMATS = tuple(oracle.MX_NAMES)  # fp8 | fp4


class Codec:
    def __init__(self, kind: str = "topk_qsgd", ratio: float = 0.01, levels: int = 127,
                 bits: int = 8, norm: str = "max", seed: int = 0, dense_below: int = 0,
                 rank: int = 4, aggregate: str = "majority", rotate: str = "none",
                 fmt: str = None, clip: float = 2.5, rows: int = None, width: float = None):
        if kind not in KINDS:
            raise ValueError(f"unknown codec {kind!r}; choose from {KINDS}")
        if kind == "powersgd" and rank not in POWERSGD_RANKS:
            raise ValueError(f"PowerSGD rank must be one of {POWERSGD_RANKS}, not {rank!r}")
        self.rank = int(rank)
        if aggregate not in VOTE_AGGREGATES:
            raise ValueError(f"vote aggregate must be one of {VOTE_AGGREGATES}, not {aggregate!r}")
        if aggregate != "majority" and kind != "vote":
            raise ValueError("the aggregate belongs to the vote codec")
        self.aggregate = aggregate
        if rotate not in SIGN_ROTATIONS:
            raise ValueError(f"sign rotation must be one of {SIGN_ROTATIONS}, not {rotate!r}")
        if rotate != "none" and kind != "sign":
            raise ValueError("the rotation belongs to the sign codec")
        self.rotate = rotate
        if fmt is not None and kind != "mx":
            raise ValueError("the element format belongs to the mx codec")
        if kind == "mx":  # the element width is the format's, whatever `bits` says
            fmt = "fp8" if fmt is None else fmt
            if fmt not in MX_FORMATS:
                raise ValueError(f"mx format must be one of {MX_FORMATS}, not {fmt!r}")
            bits = oracle.MX_NAMES[fmt]
        self.fmt = fmt
        clip = float(clip)
        if clip != oracle.TERN_CLIP and kind != "tern":
            raise ValueError("the clipping constant belongs to the tern codec")
        if not clip >= 0.0:
            raise ValueError("tern clip must be >= 0 (0: no clipping)")
        self.clip = clip
        if (rows is not None or width is not None) and kind != "sketch":
            raise ValueError("rows and width belong to the sketch codec")
        if kind == "sketch":
            rows = 3 if rows is None else rows
            width = 2.0 if width is None else float(width)
            if rows not in SKETCH_ROWS:
                raise ValueError(f"sketch rows must be one of {SKETCH_ROWS}, not {rows!r}")
            if not width > 0.0:
                raise ValueError(f"sketch width must be > 0, not {width!r}")
        self.rows, self.width = rows, width
        # the sign, vote and low-rank codecs have neither bits nor levels; tern's are fixed
        if kind not in ("sign", "powersgd", "vote", "tern", "sketch", "thresh", "intsgd") \
                and bits not in (4, 8):
            raise ValueError("bits must be 8 or 4")
        if kind in ("qsgd", "topk_qsgd"):
            lim = 127 if bits == 8 else 7
            if not 1 <= levels <= lim:
                raise ValueError(f"QSGD levels must be in [1, {lim}] for {bits}-bit codes")
        if not 0.0 < ratio <= 1.0:
            raise ValueError("top-k ratio must be in (0, 1]")
        self.kind, self.ratio, self.levels, self.bits, self.norm = kind, ratio, levels, bits, norm
        self.seed = seed
        self.dense_below = int(dense_below)
        self.plans = []
        self.layouts = []
        self.dplans = []
        self.device = None

    # -- properties -------------------------------------------------------------------------
    @property
    def allreduce(self) -> bool:
        """Dense codecs are summed by the collective itself (all-reduce)."""
        return self.kind in ("none", "fp16", "bf16")

    @property
    def wire_dtype(self):
        return {"none": torch.float32, "fp16": torch.float16, "bf16": torch.bfloat16}.get(self.kind)

    def describe(self) -> str:
        if self.kind == "topk_qsgd":
            return f"topk{self.ratio:g}+qsgd{self.bits}b(s={self.levels},{self.norm})"
        if self.kind == "qsgd":
            return f"qsgd{self.bits}b(s={self.levels},{self.norm})"
        if self.kind == "topk":
            return f"topk{self.ratio:g}"
        if self.kind == "sign":
            return "sign1b-h" if self.rotate == "hadamard" else "sign1b"
        if self.kind == "powersgd":
            return f"powersgd-r{self.rank}"
        if self.kind == "vote":
            return "vote1b"
        if self.kind == "mx":
            return "mx" + self.fmt
        if self.kind == "tern":
            return f"tern2b(c={self.clip:g})" if self.clip > 0 else "tern2b"
        if self.kind == "sketch":
            return f"sketch-r{self.rows}"
        if self.kind == "thresh":
            return f"thresh-k{self.ratio:g}"
        if self.kind == "intsgd":
            return "intsgd8"
        return self.kind

    # -- binding ----------------------------------------------------------------------------
    def bind(self, plans, device):
        self.device = torch.device(device)
        self.plans = list(plans)
        self._bound = {}  # ratio -> (plans, layouts, device plans): see set_ratio
        if self.kind == "powersgd":
            raise ValueError("the PowerSGD codec is bound by its own exchange (bind_powersgd; "
                             "--compress powersgd on the trainer)")
        if self.kind == "sketch":
            raise ValueError("the sketch codec is bound by its own exchange (bind_sketch; "
                             "--compress sketch on the trainer)")
        if self.kind == "intsgd":
            raise ValueError("the intsgd codec is bound by its own exchange (bind_intsgd; "
                             "--compress intsgd on the trainer)")
        if self.allreduce:
            self.layouts = [None] * len(self.plans)
            return self
        lk = "qsgd" if self.kind == "qsgd" else self.kind
        if self.kind in ("topk", "topk_qsgd", "thresh"):
            # the plans carry k; rebuild with this codec's ratio if needed
            self.plans = [p if (p.ratio == self.ratio and p.dense_below == self.dense_below)
                          else BucketPlan(p.numels, p.offsets, self.ratio, p.bucket_offset,
                                          p.length, self.dense_below) for p in self.plans]
        self.layouts = [Layout.build(lk, p, self.bits) for p in self.plans]
        if self.device.type == "cuda":
            if ops.hip_required():
                ops.require()
            self.dplans = [ops.DevicePlan(p, self.device) for p in self.plans]
            if self.kind == "thresh":
                # last step's threshold of every chunk row: where the next search starts.  Chunk
                # rows do not depend on the ratio, so it outlives set_ratio; the payload never
                # depends on it, so it is no part of a checkpoint
                self.thr_state = [torch.zeros(p.num_chunks, dtype=torch.int32,
                                              device=self.device) for p in self.plans]
        self._bound[self.ratio] = (self.plans, self.layouts, self.dplans)
        return self

    def set_ratio(self, ratio: float):
        """Switch a bound top-k codec to another density (top-k warm-up): the per-tensor k, the
        payload layouts and the device tables change; bindings are cached per ratio."""
        if self.kind not in ("topk", "topk_qsgd", "sketch", "thresh"):
            raise ValueError("only top-k codecs have a density")
        if not 0.0 < ratio <= 1.0:
            raise ValueError("top-k ratio must be in (0, 1]")
        if ratio == self.ratio:
            return self
        if self.kind == "sketch":  # k per tensor, and with it the table width, change
            self.ratio = ratio
            return self.bind_sketch(self.plans, self.device)
        hit = self._bound.get(ratio)
        if hit is None:
            plans = [BucketPlan(p.numels, p.offsets, ratio, p.bucket_offset, p.length,
                                self.dense_below) for p in self.plans]
            layouts = [Layout.build(self.kind, p, self.bits) for p in plans]
            dplans = ([ops.DevicePlan(p, self.device) for p in plans]
                      if self.device.type == "cuda" else [])
            hit = self._bound[ratio] = (plans, layouts, dplans)
        self.ratio = ratio
        self.plans, self.layouts, self.dplans = hit
        return self

    def payload_bytes(self, b: int) -> int:
        if self.allreduce:
            p = self.plans[b]
            return p.length * self.wire_dtype.itemsize
        return self.layouts[b].nbytes

    def dense_bytes(self, b: int) -> int:
        return self.plans[b].numel * 4

    def key(self, step: int, rank: int) -> int:
        return stream_key(self.seed, step, rank)

    def rot_key(self, b: int):
        """The rotated sign codec's key of bucket ``b`` (the same on every rank and every step);
        None without a rotation."""
        return oracle.hsign_rot_key(self.seed, b) if self.rotate == "hadamard" else None

    def _unrotated(self, what: str):
        if self.rotate != "none":
            raise ValueError(f"{what} is not rotated: it does not run with rotate="
                             f"{self.rotate!r}")

    # -- encode / decode ----------------------------------------------------------------------
    def encode(self, b: int, grad: torch.Tensor, payload: torch.Tensor, step: int, rank: int,
               resid: torch.Tensor = None, key_tensor: torch.Tensor = None, dgc: dict = None,
               ef21: bool = False, apply: dict = None):
        """Compress bucket ``b`` of the flat gradient (``grad`` = that bucket's view).  ``dgc``:
        error feedback with momentum correction (top-k codecs; ``oracle.dgc_accumulate``).
        ``apply`` (GPU top-k, a world of one): the encode also applies the decoded update
        (``ops.topk_encode``), so no decode launch follows."""
        if dgc is not None and (resid is None or self.kind not in ("topk", "topk_qsgd")):
            raise ValueError("momentum correction needs a top-k codec and a residual")
        if self.kind in ("sign", "mx", "tern", "thresh") and apply is not None:
            raise ValueError(f"the {self.kind} codec has no encode-side apply")
        if self.kind == "vote":
            raise ValueError("the vote codec sends the sign of Lion's update direction: "
                             "encode_vote, with the rank's momentum")
        plan, lay = self.plans[b], self.layouts[b]
        key = self.key(step, rank)
        on_dev = (grad[0] if isinstance(grad, (list, tuple)) else grad).is_cuda
        if ef21 and (resid is None or self.kind not in ("topk", "topk_qsgd")):
            raise ValueError("EF21 needs a top-k codec and the gradient estimate")
        if on_dev and not _FORCE_ORACLE:
            if ef21:
                raise NotImplementedError("EF21 encode on the GPU: run with EWDML_ORACLE=1")
            if self.kind == "sign":
                ops.sign_encode(self.dplans[b], grad, payload, lay, resid,
                                rot_key=self.rot_key(b))
            elif self.kind == "mx":
                ops.mx_encode(self.dplans[b], grad, payload, lay, resid)
            elif self.kind == "tern":
                ops.tern_encode(self.dplans[b], grad, payload, lay, self.clip, key, resid,
                                key_tensor)
            elif self.kind == "thresh":
                ops.thresh_encode(self.dplans[b], grad, payload, lay, resid, self.thr_state[b])
            elif self.kind == "qsgd":
                ops.qsgd_encode(self.dplans[b], grad, payload, lay, self.levels, self.norm, key,
                                resid, key_tensor)
            else:
                ops.topk_encode(self.dplans[b], grad, payload, lay, self.levels, self.norm, key,
                                resid, key_tensor, dgc=dgc, apply=apply)
            return
        if apply is not None:
            raise ValueError("the encode-side apply runs on the GPU codec only")
        if isinstance(grad, (list, tuple)):
            raise TypeError("CPU encode takes the bucket's flat gradient view")
        if self.kind == "sign":
            out = oracle.encode_sign(grad, plan, lay, resid, self.rot_key(b))
        elif self.kind == "mx":
            out = oracle.encode_mx(grad, plan, lay, resid)
        elif self.kind == "tern":
            out = oracle.encode_tern(grad, plan, lay, self.clip, key, resid)
        elif self.kind == "thresh":
            out = oracle.encode_thresh(grad, plan, lay, resid)
        elif self.kind == "qsgd":
            out = oracle.encode_qsgd(grad, plan, lay, self.levels, self.norm, key, resid)
        else:
            out = oracle.encode_topk(grad, plan, lay, self.levels, self.norm, key, resid, dgc,
                                     ef21)
        payload[:lay.nbytes].copy_(out)

    def encode_momentum(self, b: int, grad, payload: torch.Tensor, resid: torch.Tensor,
                        exp_avg: torch.Tensor, beta1: float, weight_decay: float = 0.0,
                        param: torch.Tensor = None):
        """1-bit Adam's compressed stage: the sign encode (error feedback always on) of ``exp_avg *
        beta1 + (1 - beta1) * (grad + weight_decay * param)`` of bucket ``b``; ``exp_avg`` and
        ``param`` are that bucket's views and are only read."""
        if self.kind != "sign":
            raise ValueError("the momentum encode needs the sign codec")
        self._unrotated("the momentum encode")
        if resid is None:
            raise ValueError("the momentum encode needs the residual (error feedback)")
        plan, lay = self.plans[b], self.layouts[b]
        on_dev = (grad[0] if isinstance(grad, (list, tuple)) else grad).is_cuda
        if on_dev and not _FORCE_ORACLE:
            ops.sign_encode_momentum(self.dplans[b], grad, payload, lay, resid, exp_avg, beta1,
                                     weight_decay, param)
            return
        if isinstance(grad, (list, tuple)):
            raise TypeError("CPU encode takes the bucket's flat gradient view")
        out = oracle.encode_sign_momentum(grad, plan, lay, resid, exp_avg, beta1, weight_decay,
                                          param)
        payload[:lay.nbytes].copy_(out)

    # -- Distributed Lion's vote (optim/flat.py FlatLion): one launch per bucket and side ---------
    def encode_vote(self, b: int, grad, payload: torch.Tensor, exp_avg: torch.Tensor,
                    betas, step: int, rank: int, step_tensor: torch.Tensor = None):
        """This rank's vote of bucket ``b``: one bit per element, the sign of ``exp_avg * beta1 +
        (1 - beta1) * grad``; ``exp_avg`` (the rank's own momentum, that bucket's view) then moves
        with ``beta2``.  ``step``: the 1-based step of the exact-zero dither (on the GPU
        ``step_tensor``, the optimizer's device counter, is read instead)."""
        if self.kind != "vote":
            raise ValueError("the vote encode needs the vote codec")
        plan, lay = self.plans[b], self.layouts[b]
        b1, b2 = betas
        on_dev = (grad[0] if isinstance(grad, (list, tuple)) else grad).is_cuda
        if on_dev and not _FORCE_ORACLE:
            ops.lion_encode(self.dplans[b], grad, payload, lay, exp_avg, b1, b2, step, rank,
                            step_tensor=step_tensor)
            return
        if isinstance(grad, (list, tuple)):
            raise TypeError("CPU encode takes the bucket's flat gradient view")
        payload[:lay.nbytes].copy_(oracle.encode_vote(grad, plan, lay, exp_avg, b1, b2, step,
                                                      rank))

    def decode_apply_vote(self, b: int, recv: torch.Tensor, param: torch.Tensor, hp: dict,
                          shadow=None, key_state=None, rank: int = 0):
        """Count the N received votes of bucket ``b`` and step its parameters by the majority (or
        the average, ``aggregate``) of the signs.  ``hp``: ``FlatLion.hparams()``."""
        if self.kind != "vote":
            raise ValueError("the vote apply needs the vote codec")
        plan, lay = self.plans[b], self.layouts[b]
        inv_n = 1.0 / recv.shape[0]
        if recv.is_cuda and not _FORCE_ORACLE:
            ops.lion_vote_apply(self.dplans[b], recv, lay, param, hp["lr"], hp["weight_decay"],
                                self.aggregate, inv_n, shadow=shadow, lr_tensor=hp.get("lr_t"),
                                key_state=key_state, key_seed=self.seed, key_rank=rank)
            return
        oracle.vote_apply(recv, plan, lay, param, hp["lr"], hp["weight_decay"], self.aggregate,
                          inv_n)

    # -- two-stage sign all-reduce (parallel/twostage.py): three launches per bucket ------------
    def bind_twostage(self, ts_plans, device):
        """Bind the buckets' :class:`TwoStagePlan` s.  On the GPU every bucket gets its slot
        tables and every non-empty shard its chunk table (any rank may be asked to own any shard:
        the kernel tests drive all of them from one process)."""
        if self.kind not in ("sign", "vote"):
            raise ValueError("the two-stage exchange needs the sign codec (or, for the two-stage "
                             "vote, the vote codec)")
        self._unrotated("the two-stage exchange (its owner re-encode would need a transform pair "
                        "of its own)")
        if self.kind == "vote" and self.aggregate != "majority":
            raise ValueError("the two-stage vote returns one bit per element: a mean does not "
                             "fit it (aggregate must be majority)")
        self.device = torch.device(device)
        self.ts = list(ts_plans)
        if any(getattr(t, "kind", "sign") != self.kind for t in self.ts):
            raise ValueError(f"the {self.kind} codec binds two-stage plans of kind {self.kind!r}")
        self.ts_dev = self.ts_shard_dev = None
        if self.device.type == "cuda" and not _FORCE_ORACLE:
            if ops.hip_required():
                ops.require()
            self.ts_dev = [ops.SignSlots(t, self.device) for t in self.ts]
            self.ts_shard_dev = [[None if sp is None else ops.SignTables(sp, self.device)
                                  for _, _, sp, _, _ in t.shards] for t in self.ts]
        return self

    def _ts_kernel(self, t: torch.Tensor) -> bool:
        return t.is_cuda and not _FORCE_ORACLE

    def ts_encode(self, b: int, grad: torch.Tensor, rows: torch.Tensor, resid: torch.Tensor,
                  mom: dict = None):
        """Push: sign-encode (error feedback through the worker residual ``resid``) every shard
        of bucket ``b`` of the flat gradient view ``grad`` into its row of ``rows`` (``[N, P]``).
        ``mom`` (``exp_avg``, ``beta1``, ``weight_decay``, ``param``): 1-bit Adam's momentum
        encode instead.  One launch on the GPU."""
        ts = self.ts[b]
        if resid is None:
            raise ValueError("the two-stage push always runs with error feedback")
        if self._ts_kernel(grad):
            sl = self.ts_dev[b]
            if mom is None:
                ops.sign_encode(sl, grad, rows, None, resid, slots=sl)
            else:
                ops.sign_encode_momentum(sl, grad, rows, None, resid, mom["exp_avg"],
                                         mom["beta1"], mom.get("weight_decay", 0.0),
                                         mom.get("param"), slots=sl)
            return
        for r, (s0, ln, sp, lay, _) in enumerate(ts.shards):
            if sp is None:
                continue
            sl = slice(s0, s0 + ln)
            if mom is None:
                out = oracle.encode_sign(grad[sl], sp, lay, resid[sl])
            else:
                out = oracle.encode_sign_momentum(grad[sl], sp, lay, resid[sl], mom["exp_avg"][sl],
                                                  mom["beta1"], mom.get("weight_decay", 0.0),
                                                  None if mom.get("param") is None
                                                  else mom["param"][sl])
            rows[r, :lay.nbytes].copy_(out)

    def ts_reduce_encode(self, b: int, r: int, recv: torch.Tensor, out: torch.Tensor, inv_n: float,
                         sresid: torch.Tensor):
        """Owner step of shard ``r`` of bucket ``b``: average the N received rows ``recv`` (``[N,
        P]``), add the server residual ``sresid`` (shard-relative, updated in place) and
        sign-encode again into the row ``out``.  One launch on the GPU."""
        _, ln, sp, lay, _ = self.ts[b].shards[r]
        if sp is None:
            raise ValueError("an empty shard has no owner step")
        if self._ts_kernel(recv):
            ops.sign_reduce_encode(self.ts_shard_dev[b][r], recv, lay, inv_n, sresid, out)
            return
        out[:lay.nbytes].copy_(oracle.sign_reduce_encode(recv, sp, lay, inv_n, sresid[:ln]))

    def _ts_decoded(self, b: int, rows: torch.Tensor) -> torch.Tensor:
        """Oracle pull: every shard's row decoded into a bucket-length fp32 vector."""
        ts = self.ts[b]
        g = torch.zeros(ts.plan.length, dtype=torch.float32, device=rows.device)
        for r, (s0, ln, sp, lay, _) in enumerate(ts.shards):
            if sp is not None:
                g[s0:s0 + ln] = oracle.decode_sum(rows[r:r + 1, :lay.nbytes], sp, lay, 0, 1.0)
        return g

    def ts_decode_apply_sgd(self, b: int, rows: torch.Tensor, param: torch.Tensor,
                            mom: torch.Tensor, hp: dict, first: bool, grad_out=None, shadow=None,
                            key_state=None, rank: int = 0):
        """Pull: decode every owner's row of the gathered ``rows`` (``[N, P]``, already averaged:
        scale 1) and take the fused SGD step of bucket ``b``; ``param`` None: write the decoded
        mean to ``grad_out`` only.  One launch on the GPU."""
        if param is not None and mom is None and hp["momentum"] != 0:
            raise ValueError("a momentum step needs the momentum buffer")
        ts = self.ts[b]
        if self._ts_kernel(rows):
            sl = self.ts_dev[b]
            ops.sign_decode_apply(sl, rows, None, grad_out=grad_out, grad_scale=1.0,
                                  key_state=key_state, key_seed=self.seed, key_rank=rank,
                                  slots=sl, **_sgd_kw(hp, first, shadow, param, mom))
            return
        g = self._ts_decoded(b, rows)
        if grad_out is not None:
            grad_out[:ts.plan.length].copy_(g)
        if param is None:
            return
        for off, n in zip(ts.plan.offsets, ts.plan.numels):
            oracle.sgd_apply(param[off:off + n], None if mom is None else mom[off:off + n],
                             g[off:off + n], hp["lr"], hp["momentum"], hp["dampening"],
                             hp["weight_decay"], hp["nesterov"], first)

    def ts_decode_apply_onebit(self, b: int, rows: torch.Tensor, param: torch.Tensor,
                               exp_avg: torch.Tensor, exp_avg_sq: torch.Tensor, hp: dict,
                               shadow=None, key_state=None, rank: int = 0):
        """Pull of 1-bit Adam: ``exp_avg`` = the decoded rows (``inv_n`` = 1, the owners
        averaged), then the frozen-variance step of bucket ``b``.  One launch on the GPU."""
        ts = self.ts[b]
        if self._ts_kernel(rows):
            sl = self.ts_dev[b]
            b1, b2 = hp["betas"]
            ops.sign_decode_onebit(sl, rows, None, param, exp_avg, exp_avg_sq, 1.0,
                                   hp["lr_step"], hp["eps"], b1, b2, hp["freeze_step"],
                                   shadow=shadow, step=hp.get("step_t"), lr=hp["lr"],
                                   lr_tensor=hp.get("lr_t"), key_state=key_state,
                                   key_seed=self.seed, key_rank=rank, slots=sl)
            return
        for r, (s0, ln, sp, lay, _) in enumerate(ts.shards):
            if sp is not None:
                sl = slice(s0, s0 + ln)
                oracle.onebit_adam_apply(rows[r:r + 1, :lay.nbytes], sp, lay, param[sl],
                                         exp_avg[sl], exp_avg_sq[sl], 1.0, hp["lr_step"],
                                         hp["eps"])

    # -- two-stage vote (parallel/twostage.py TwoStageVoteExchange): three launches per bucket ------
    def ts_encode_vote(self, b: int, grad: torch.Tensor, rows: torch.Tensor,
                       exp_avg: torch.Tensor, betas, step: int, rank: int,
                       step_tensor: torch.Tensor = None):
        """Push: this rank's vote (``encode_vote``) on every shard of bucket ``b`` of the flat
        gradient view ``grad``, shard r into row r of ``rows`` (``[N, P]``); ``exp_avg`` (the
        bucket's view of the rank's own momentum) then moves with ``beta2``.  One launch on the
        GPU."""
        if self.kind != "vote":
            raise ValueError("the vote push needs the vote codec")
        b1, b2 = betas
        if self._ts_kernel(rows):
            sl = self.ts_dev[b]
            ops.lion_encode(sl, grad, rows, None, exp_avg, b1, b2, step, rank,
                            step_tensor=step_tensor, slots=sl)
            return
        if isinstance(grad, (list, tuple)):
            raise TypeError("CPU encode takes the bucket's flat gradient view")
        for r, (s0, ln, sp, lay, _) in enumerate(self.ts[b].shards):
            if sp is not None:
                rows[r, :lay.nbytes].copy_(oracle.encode_vote(
                    grad[s0:s0 + ln], sp, lay, exp_avg[s0:s0 + ln], b1, b2, step, rank))

    def ts_vote_reduce(self, b: int, r: int, recv: torch.Tensor, out: torch.Tensor):
        """Owner step of shard ``r`` of bucket ``b``: the N votes ``recv`` (``[N, P]``) become
        one bit per element again in the row ``out``; a tie takes row ``r``'s (the owner's own)
        vote.  One launch on the GPU; no parameter is touched."""
        if self.kind != "vote":
            raise ValueError("the vote owner step needs the vote codec")
        _, _, sp, lay, _ = self.ts[b].shards[r]
        if sp is None:
            raise ValueError("an empty shard has no owner step")
        if self._ts_kernel(recv):
            ops.vote_reduce(self.ts_shard_dev[b][r], recv, lay, r, out)
            return
        out[:lay.nbytes].copy_(oracle.vote_reduce(recv, sp, lay, r))

    def ts_decode_apply_vote(self, b: int, rows: torch.Tensor, param: torch.Tensor, hp: dict,
                             shadow=None, key_state=None, rank: int = 0):
        """Pull: every owner's row of the gathered ``rows`` (``[N, P]``) is the direction of its
        shard (``d = 1 - 2 * bit``) and bucket ``b``'s parameters take Lion's step.  ``hp``:
        ``FlatLion.hparams()``.  One launch on the GPU."""
        if self.kind != "vote":
            raise ValueError("the vote pull needs the vote codec")
        if self._ts_kernel(rows):
            sl = self.ts_dev[b]
            ops.lion_vote_apply(sl, rows, None, param, hp["lr"], hp["weight_decay"], "majority",
                                1.0, shadow=shadow, lr_tensor=hp.get("lr_t"),
                                key_state=key_state, key_seed=self.seed, key_rank=rank, slots=sl)
            return
        for r, (s0, ln, sp, lay, _) in enumerate(self.ts[b].shards):
            if sp is not None:
                oracle.vote_apply(rows[r:r + 1, :lay.nbytes], sp, lay, param[s0:s0 + ln],
                                  hp["lr"], hp["weight_decay"], "majority", 1.0)

    # -- PowerSGD (parallel/powersgd.py): four launches per bucket --------------------------------
    def bind_powersgd(self, lr_plans, device):
        """Bind the buckets' :class:`LowRankPlan` s (and, on the GPU, their device tables)."""
        if self.kind != "powersgd":
            raise ValueError("the PowerSGD exchange needs the powersgd codec")
        if any(p.rank != self.rank for p in lr_plans):
            raise ValueError("plans of another rank than the codec's")
        self.device = torch.device(device)
        self.lr_plans = list(lr_plans)
        self.lr_dev = None
        if self.device.type == "cuda" and not _FORCE_ORACLE:
            if ops.hip_required():
                ops.require()
            self.lr_dev = [ops.LowRankTables(p, self.device) for p in self.lr_plans]
        return self

    def ps_project(self, b: int, grad: torch.Tensor, resid: torch.Tensor, q: torch.Tensor,
                   p: torch.Tensor):
        """``resid <- M = grad + resid`` (compressed tensors) and ``p`` = the ``M Q`` factors of
        bucket ``b`` followed by its dense gradients.  One launch on the GPU."""
        if self._ts_kernel(grad):
            ops.psgd_project(self.lr_dev[b], grad, resid, q, p)
            return
        lrp = self.lr_plans[b]
        p[:lrp.p_floats].copy_(oracle.powersgd_project(grad, resid, q, lrp))

    def ps_orthogonalize(self, b: int, p: torch.Tensor, inv_n: float):
        """The summed P factors of bucket ``b`` averaged and orthogonalised in place."""
        if self._ts_kernel(p):
            ops.psgd_orth(self.lr_dev[b], p, inv_n)
            return
        oracle.powersgd_orthogonalize(p, self.lr_plans[b], inv_n)

    def ps_backproject(self, b: int, resid: torch.Tensor, p: torch.Tensor, q: torch.Tensor):
        """``q`` = the ``M^T P`` factors of bucket ``b``.  One launch on the GPU."""
        if self._ts_kernel(p):
            ops.psgd_backproject(self.lr_dev[b], resid, p, q)
            return
        lrp = self.lr_plans[b]
        q[:lrp.q_floats].copy_(oracle.powersgd_backproject(resid, p, lrp))

    def ps_decode_apply_sgd(self, b: int, resid: torch.Tensor, p: torch.Tensor, q: torch.Tensor,
                            q_out: torch.Tensor, inv_n: float, param: torch.Tensor,
                            mom: torch.Tensor, hp: dict, first: bool, grad_out=None, shadow=None):
        """Reconstruct ``g^`` of bucket ``b`` from ``p`` and the summed ``q`` (``q_out = q *
        inv_n``, the next warm start), ``resid <- M - g^`` and the fused SGD step; ``param`` None:
        write ``g^`` to ``grad_out`` only.  One launch on the GPU."""
        if param is not None and mom is None and hp["momentum"] != 0:
            raise ValueError("a momentum step needs the momentum buffer")
        if self._ts_kernel(p):
            ops.psgd_decode_apply(self.lr_dev[b], resid, p, q, q_out, inv_n, grad_out=grad_out,
                                  **_sgd_kw(hp, first, shadow, param, mom))
            return
        lrp = self.lr_plans[b]
        qa = oracle.powersgd_reconstruct_apply(resid, p, q, lrp, inv_n, param, mom, hp, first,
                                               grad_out)
        q_out[:lrp.q_floats].copy_(qa)

    # -- count sketch (parallel/sketch.py): stage + table, estimate + select + gather, apply -------
    def bind_sketch(self, plans, device):
        """Bind the buckets' top-k plans at this codec's density: per bucket the ``topk`` payload
        layout (its index sections carry the selection, its values the second all-reduce) and
        the :class:`SketchPlan`; on the GPU their device tables.  Called again by ``set_ratio``
        (density warm-up: k, W and the layouts change); bindings are cached per ratio."""
        if self.kind != "sketch":
            raise ValueError("the sketch exchange needs the sketch codec")
        self.device = torch.device(device)
        if not hasattr(self, "_bound"):
            self._bound = {}
        hit = self._bound.get(self.ratio)
        if hit is None:
            bplans = [BucketPlan(p.numels, p.offsets, self.ratio, p.bucket_offset, p.length,
                                 self.dense_below) for p in plans]
            layouts = [Layout.build("topk", p) for p in bplans]
            sk = [SketchPlan(p, self.rows, self.width, *oracle.sketch_keys(self.seed, b))
                  for b, p in enumerate(bplans)]
            dplans, sk_dev = [], None
            if self.device.type == "cuda" and not _FORCE_ORACLE:
                if ops.hip_required():
                    ops.require()
                dplans = [ops.DevicePlan(p, self.device) for p in bplans]
                sk_dev = [ops.SketchTables(t, self.device) for t in sk]
            hit = self._bound[self.ratio] = (bplans, layouts, dplans, sk, sk_dev)
        self.plans, self.layouts, self.dplans, self.sk, self.sk_dev = hit
        return self

    def sk_sketch(self, b: int, grad: torch.Tensor, resid: torch.Tensor, table: torch.Tensor):
        """``resid <- acc = grad + resid`` on the sketched tensors of bucket ``b`` and ``table`` =
        the count sketch of ``acc``.  Two launches on the GPU."""
        if self._ts_kernel(grad):
            ops.sketch_stage(self.sk_dev[b], grad, resid)
            ops.sketch_accum(self.sk_dev[b], resid, table)
            return
        sp = self.sk[b]
        oracle.sketch_stage(grad, resid, sp)
        table[:sp.table_floats].copy_(oracle.sketch_accumulate(resid, sp))

    def sk_select_gather(self, b: int, table: torch.Tensor, est: torch.Tensor,
                         grad: torch.Tensor, resid: torch.Tensor, payload: torch.Tensor):
        """From the summed ``table`` of bucket ``b``: the estimate (``est``, a bucket-length
        scratch whose dense tensors and pads stay 0), the top-k selection of the estimate into
        ``payload`` and this rank's own values at the selected coordinates in its values section,
        cleared from ``resid``.  The estimate, the exact top-k passes and the gather on the GPU."""
        sp, lay = self.sk[b], self.layouts[b]
        if self._ts_kernel(table):
            st, dp = self.sk_dev[b], self.dplans[b]
            ops.sketch_estimate(st, table, est)
            ops.topk_encode(dp, est, payload, lay, self.levels, "max", 0, predict=False)
            ops.sketch_gather(st, dp, payload, lay, grad, resid)
            return
        est[:sp.plan.length].copy_(oracle.sketch_estimate(table, sp))
        payload[:lay.nbytes].copy_(oracle.sketch_select(est[:sp.plan.length], sp, lay))
        oracle.sketch_gather(payload, grad, resid, sp, lay)

    def sk_values(self, b: int, payload: torch.Tensor) -> torch.Tensor:
        """The fp32 values section of bucket ``b``'s payload: what the second all-reduce sums."""
        lay = self.layouts[b]
        return payload[lay.codes:lay.codes + 4 * self.plans[b].total_k].view(torch.float32)

    def sk_decode_apply_sgd(self, b: int, payload: torch.Tensor, inv_n: float, param, mom, hp,
                            first: bool, grad_out=None, shadow=None):
        """``g^ = vals * inv_n`` at the selected coordinates of bucket ``b`` and 0 elsewhere, and
        the fused SGD step (``param`` None: ``g^`` to ``grad_out`` only): the plain top-k decode
        of the one summed payload."""
        recv = payload[:self.layouts[b].nbytes].unsqueeze(0)
        if param is None:
            self.decode(b, recv, grad_out, inv_n)
            return
        self.decode_apply_sgd(b, recv, inv_n, param, mom, hp, first, grad_out=grad_out,
                              shadow=shadow)

    # -- IntSGD (parallel/intsgd.py): encode, int8 all-reduce, decode + step, the scale rule ------
    def bind_intsgd(self, plans, device, world: int):
        """Bind the buckets' plans for a job of ``world`` ranks: per bucket the ``intsgd`` layout
        (one byte per position); model-wide the scale state, the saturation counts and the
        update-norm partials, one entry per chunk row in bucket order, then chunk order."""
        if self.kind != "intsgd":
            raise ValueError("the IntSGD exchange needs the intsgd codec")
        self.device = torch.device(device)
        self.world, self.q = int(world), oracle.intsgd_q(world)
        self.plans = list(plans)
        self.layouts = [Layout.build("intsgd", p) for p in self.plans]
        self.dplans = []
        if self.device.type == "cuda" and not _FORCE_ORACLE:
            if ops.hip_required():
                ops.require()
            self.dplans = [ops.DevicePlan(p, self.device) for p in self.plans]
        self.int_chunk0, n = [], 0
        for p in self.plans:
            self.int_chunk0.append(n)
            n += p.num_chunks
        self.int_numel = sum(p.numel for p in self.plans)
        self.int_state = IntSGDState(self.device)
        self.int_sat = torch.zeros(n, dtype=torch.int32, device=self.device)
        self.int_partials = torch.zeros(n, dtype=torch.float32, device=self.device)
        return self

    def _int_rows(self, b: int, t: torch.Tensor) -> torch.Tensor:
        c0 = self.int_chunk0[b]
        return t[c0:c0 + self.plans[b].num_chunks]

    def int_encode(self, b: int, grad: torch.Tensor, payload: torch.Tensor, step: int, rank: int,
                   resid: torch.Tensor = None, key_tensor: torch.Tensor = None):
        """The int8 codes of bucket ``b`` under the current scale and its rows of ``int_sat``;
        ``resid`` (error feedback) is updated in place.  One launch on the GPU."""
        plan, lay, key = self.plans[b], self.layouts[b], self.key(step, rank)
        sat = self._int_rows(b, self.int_sat)
        if self._ts_kernel(payload):
            ops.int_encode(self.dplans[b], grad, payload, lay, self.int_state.buf, sat, self.q,
                           key, resid, key_tensor)
            return
        v = self.int_state.values()
        out, s = oracle.encode_intsgd(grad, plan, lay, v["alpha"], v["inv_a"], self.q, key, resid)
        payload[:lay.nbytes].copy_(out)
        sat.copy_(s)

    def int_decode_apply(self, b: int, summed: torch.Tensor, param: torch.Tensor,
                         mom: torch.Tensor, hp: dict, first: bool, shadow=None, key_state=None,
                         rank: int = 0):
        """The fused receive side of bucket ``b`` on its summed codes: decode with ``inv_na``,
        the SGD step, and the bucket's rows of ``int_partials``.  One launch on the GPU."""
        if mom is None and hp["momentum"] != 0:
            raise ValueError("a momentum step needs the momentum buffer")
        plan, lay = self.plans[b], self.layouts[b]
        part = self._int_rows(b, self.int_partials)
        if self._ts_kernel(summed):
            ops.int_decode_apply(self.dplans[b], summed[:lay.nbytes], lay, self.int_state.buf,
                                 part, key_state=key_state, key_seed=self.seed, key_rank=rank,
                                 **_sgd_kw(hp, first, shadow, param, mom))
            return
        oracle.intsgd_apply(summed, plan, lay, self.int_state.values()["inv_na"], param, mom, hp,
                            first, part)

    def int_update_norm(self, b: int, param: torch.Tensor, prev: torch.Tensor):
        """Bucket ``b``'s rows of ``int_partials`` from its parameters and a previous copy."""
        part = self._int_rows(b, self.int_partials)
        if self._ts_kernel(param):
            ops.int_update_norm(self.dplans[b], param, prev, part)
            return
        part.copy_(oracle.intsgd_update_partials(param, prev, self.plans[b]))

    def int_alpha(self, lr: float, lr_tensor=None):
        """The scale rule after a step (every bucket's partials are in place).  One single-block
        launch on the GPU."""
        if self._ts_kernel(self.int_partials):
            ops.int_alpha(self.int_partials, self.int_state.buf, lr, self.int_numel, self.world,
                          lr_tensor=lr_tensor)
            return
        v = self.int_state.values()
        self.int_state.load(oracle.intsgd_alpha(self.int_partials, v["r"], v["steps"], lr,
                                                self.int_numel, self.world))

    def decode_apply_onebit(self, b: int, recv: torch.Tensor, inv_n: float, param: torch.Tensor,
                            exp_avg: torch.Tensor, exp_avg_sq: torch.Tensor, hp: dict,
                            shadow=None, key_state=None, rank: int = 0):
        """1-bit Adam's fused decode -> ``exp_avg = mean`` -> frozen-variance step of bucket ``b``
        (one kernel on the GPU).  ``hp``: ``FlatOnebitAdam.hparams()`` (``lr_step`` of this step;
        on the GPU ``step_t`` / ``lr_t`` make the kernel derive it)."""
        if self.kind != "sign":
            raise ValueError("the 1-bit Adam step needs the sign codec")
        self._unrotated("1-bit Adam's fused decode")
        plan, lay = self.plans[b], self.layouts[b]
        if recv.is_cuda and not _FORCE_ORACLE:
            b1, b2 = hp["betas"]
            ops.sign_decode_onebit(self.dplans[b], recv, lay, param, exp_avg, exp_avg_sq, inv_n,
                                   hp["lr_step"], hp["eps"], b1, b2, hp["freeze_step"],
                                   shadow=shadow, step=hp.get("step_t"), lr=hp["lr"],
                                   lr_tensor=hp.get("lr_t"), key_state=key_state,
                                   key_seed=self.seed, key_rank=rank)
            return
        oracle.onebit_adam_apply(recv, plan, lay, param, exp_avg, exp_avg_sq, inv_n,
                                 hp["lr_step"], hp["eps"])

    def decode_apply_onebit_lamb(self, b: int, recv: torch.Tensor, inv_n: float,
                                 param: torch.Tensor, exp_avg: torch.Tensor,
                                 exp_avg_sq: torch.Tensor, exp_avg_sq_fresh: torch.Tensor,
                                 hp: dict, shadow=None, key_state=None, rank: int = 0):
        """1-bit LAMB's receive side of bucket ``b``: ``exp_avg`` = the mean of the decoded
        momenta, the fresh variance, the per-tensor factor and the trust-ratio step (two kernels
        on the GPU, ``oracle.onebit_lamb_apply`` on the CPU).  ``hp``:
        ``FlatOnebitLamb.hparams(start, length)`` of the bucket (on the GPU ``step_t`` / ``lr_t``
        make the kernels read the step and the lr from device memory)."""
        if self.kind != "sign":
            raise ValueError("the 1-bit LAMB step needs the sign codec")
        self._unrotated("1-bit LAMB's fused decode")
        plan, lay = self.plans[b], self.layouts[b]
        kw = dict(lr=hp["lr"], eps=hp["eps"], freeze_step=hp["freeze_step"],
                  factor_min=hp["factor_min"], factor_max=hp["factor_max"],
                  factor_threshold=hp["factor_threshold"])
        t = hp["t"]
        if recv.is_cuda and not _FORCE_ORACLE:
            ops.onebit_lamb_step(hp["tables"](self.dplans[b]), recv, lay, param, exp_avg,
                                 exp_avg_sq, exp_avg_sq_fresh, inv_n, betas=hp["betas"],
                                 weight_decay=hp["weight_decay"], t=t, step=hp.get("step_t"),
                                 lr_tensor=hp.get("lr_t"), shadow=shadow, key_state=key_state,
                                 key_seed=self.seed, key_rank=rank, **kw)
            return
        b1, b2 = hp["betas"]
        fac = hp["factors"]
        ratios, factors = oracle.onebit_lamb_apply(
            recv, plan, lay, param, exp_avg, exp_avg_sq, exp_avg_sq_fresh, hp["tensors"],
            hp["r_frozen"], fac[(t - 1) & 1], inv_n, b1=b1, b2=b2, wd=hp["weight_decay"], step=t,
            **kw)
        hp["ratio"].copy_(ratios)
        fac[t & 1].copy_(factors)

    def _gpu_decode(self, b: int, recv: torch.Tensor, **kw):
        """The codec's ``ops.*_decode_apply`` on bucket ``b``; ``kw``: what to do with the mean."""
        dp, lay = self.dplans[b], self.layouts[b]
        if self.kind == "sign":
            ops.sign_decode_apply(dp, recv, lay, rot_key=self.rot_key(b), **kw)
        elif self.kind == "mx":
            ops.mx_decode_apply(dp, recv, lay, **kw)
        elif self.kind == "tern":
            ops.tern_decode_apply(dp, recv, lay, **kw)
        elif self.kind == "thresh":
            ops.thresh_decode_apply(dp, recv, lay, **kw)
        else:
            fn = ops.qsgd_decode_apply if self.kind == "qsgd" else ops.topk_decode_apply
            fn(dp, recv, lay, self.levels, **kw)

    def decode(self, b: int, recv: torch.Tensor, out: torch.Tensor, scale: float):
        """``out`` (bucket view) = scale * sum over ranks of the decoded payloads in ``recv``."""
        if self.kind == "vote":
            raise ValueError("a vote carries no magnitudes: there is no gradient to decode "
                             "(decode_apply_vote steps the parameters)")
        plan, lay = self.plans[b], self.layouts[b]
        if recv.is_cuda and not _FORCE_ORACLE:
            self._gpu_decode(b, recv, grad_out=out, grad_scale=scale)
            return
        out[:plan.length].copy_(oracle.decode_sum(recv, plan, lay, self.levels, scale,
                                                  self.rot_key(b)))

    def decode_apply_sgd(self, b: int, recv: torch.Tensor, scale: float, param: torch.Tensor,
                         mom: torch.Tensor, hp: dict, first: bool, grad_out=None, shadow=None,
                         key_state=None, rank: int = 0):
        """Fused decode -> average -> SGD step of bucket ``b`` (one kernel on the GPU).
        ``key_state`` (device int32 {step, key}): also advance the RNG key to the next step.
        ``mom`` may be None with ``hp["momentum"] == 0`` (momentum-corrected error feedback: the
        momentum ran on the sender, the update is p -= lr * mean)."""
        if mom is None and hp["momentum"] != 0:
            raise ValueError("a momentum step needs the momentum buffer")
        plan, lay = self.plans[b], self.layouts[b]
        if recv.is_cuda and not _FORCE_ORACLE:
            self._gpu_decode(b, recv, grad_out=grad_out, grad_scale=scale, key_state=key_state,
                             key_seed=self.seed, key_rank=rank,
                             **_sgd_kw(hp, first, shadow, param, mom))
            return
        g = oracle.decode_sum(recv, plan, lay, self.levels, scale, self.rot_key(b))
        if grad_out is not None:
            grad_out[:plan.length].copy_(g)
        for off, n in zip(plan.offsets, plan.numels):
            oracle.sgd_apply(param[off:off + n], None if mom is None else mom[off:off + n],
                             g[off:off + n], hp["lr"],
                             hp["momentum"], hp["dampening"], hp["weight_decay"],
                             hp["nesterov"], first)


class IntSGDState:
    """IntSGD's scale state of one model, 32 bytes in the memory of ``device`` (the layout of
    ``ops/csrc/intsgd_codec.hip IntState``): fp64 ``{r, S of the last step}``, fp32 ``{alpha,
    inv_a, inv_na}`` and the int32 count of steps the rule has run.  The kernels read and write
    it in place, so a captured step follows the scale."""

    FIELDS = ("r", "s_last", "alpha", "inv_a", "inv_na", "steps")

    def __init__(self, device):
        self.buf = torch.zeros(ops.INTSGD_STATE_BYTES, dtype=torch.uint8, device=device)

    @staticmethod
    def _views(buf):
        return (buf[:16].view(torch.float64), buf[16:28].view(torch.float32),
                buf[28:32].view(torch.int32))

    def values(self) -> dict:
        """The state as Python numbers (synchronises on the GPU)."""
        d, f, i = self._views(self.buf.cpu())
        return dict(r=float(d[0]), s_last=float(d[1]), alpha=float(f[0]), inv_a=float(f[1]),
                    inv_na=float(f[2]), steps=int(i[0]))

    def load(self, v: dict):
        host = torch.zeros(ops.INTSGD_STATE_BYTES, dtype=torch.uint8)
        d, f, i = self._views(host)
        d[0], d[1] = float(v["r"]), float(v.get("s_last", 0.0))
        f[0], f[1], f[2] = float(v["alpha"]), float(v["inv_a"]), float(v["inv_na"])
        i[0] = int(v["steps"])
        self.buf.copy_(host)


def _sgd_kw(hp: dict, first: bool, shadow, param, mom) -> dict:
    """The fused SGD step's keywords of ``ops.*_decode_apply`` from ``FlatSGD.hparams()``
    (``param`` None: no step, the decoded mean goes to ``grad_out`` only)."""
    if param is None:
        return {}
    return dict(param=param, mom=mom, lr=hp["lr"], momentum=hp["momentum"],
                dampening=hp["dampening"], weight_decay=hp["weight_decay"],
                nesterov=hp["nesterov"], first=first, shadow=shadow, lr_tensor=hp.get("lr_t"))


def make_codec(kind: str = "topk_qsgd", **kw) -> Codec:
    return Codec(kind, **kw)
