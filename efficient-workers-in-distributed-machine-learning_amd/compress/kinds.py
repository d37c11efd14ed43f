"""What each codec kind is and what it runs with: one :class:`Kind` per ``--compress`` value.

``Config.resolved()`` (flag defaults, refusals, orphan flags, ``--pull-compress``), ``Codec``
(validation, ``describe``, binding, the encode / decode dispatch), the trainer and the Horovod
wrapper read this table; a new codec is one entry here plus its kernels, launchers and oracle.
"""
from dataclasses import dataclass
from typing import Callable, NamedTuple, Optional

import torch

from .. import ops
from . import oracle
from .plan import POWERSGD_RANKS, SKETCH_ROWS

MX_FORMATS = tuple(oracle.MX_NAMES)  # fp8 | fp4


class Flag(NamedTuple):
    """A command-line flag that belongs to one kind: ``--mx-format`` is ``Config.mx_format``."""
    field: str
    kw: Optional[str]  # the Codec keyword it becomes (None: the exchange's business, not the codec's)
    default: object

    @property
    def option(self) -> str:
        return "--" + self.field.replace("_", "-")


class OwnExchange(NamedTuple):
    """A kind bound by an exchange of its own (``Codec.bind_<kind>``), not by ``Codec.bind``."""
    label: str  # the codec's name in Codec.bind's refusal
    no_wrapper: str  # why Horovod's DistributedOptimizer cannot run it


@dataclass(frozen=True)
class Kind:
    name: str
    describe: Callable  # codec -> its short name in logs and summaries
    # dense kinds are summed by the collective itself, in this dtype; None: the kind has a payload
    wire_dtype: Optional[torch.dtype] = None
    # bound by its own exchange: Codec.bind refuses it, the trainer hands it flat gradient views,
    # never asks plan_graph_mode for a mode and runs split graphs under --hip-graph auto
    own_exchange: Optional[OwnExchange] = None
    bits: bool = False  # the constructor checks `bits` (the payload layout reads it)
    levels: bool = False  # ... and `levels`
    density: bool = False  # k per tensor from ratio / dense_below: set_ratio, plans rebuilt in bind
    # (codec, b, grad, payload, key, resid, key_tensor, dgc, apply): the ops.*_encode launch
    gpu_encode: Optional[Callable] = None
    # (codec, b, grad, key, resid, dgc, ef21) -> payload bytes: the oracle.encode_* call
    cpu_encode: Optional[Callable] = None
    # (codec, b, recv, **kw): the ops.*_decode_apply launch; kw: what to do with the mean
    gpu_decode: Optional[Callable] = None
    # ---- command line (Config.resolved) ----------------------------------------------------------
    flags: tuple = ()  # the Flags the kind owns: filled with their defaults, refused without it
    ef_default: Optional[bool] = None  # --error-feedback unset; None: the top-k / sign rule
    # --pull-compress K is refused when the command line resolves (the older kinds without a
    # parameter-server form fail in the parameter server itself)
    no_ps_form: bool = False
    # (condition on the Config, reason) in order: the first that holds is raised as
    # "--compress K " + reason.format(c=config)
    refusals: tuple = ()
    auto_graph: Optional[str] = None  # what the command line resolves --hip-graph auto to


# ---- refusals that several kinds share: (condition, reason) -------------------------------------
def _topology(why):
    return lambda c: c.topology != "allgather", why


def _local(why):
    return lambda c: c.sync_every > 1, why


def _best(why):
    return lambda c: c.select_best, why


def _no_ef(why):
    return lambda c: not c.error_feedback, why


def _predivide(why):
    return lambda c: c.predivide != 1.0, why + " --predivide other than 1"


def _one_graph(what):
    return (lambda c: c.hip_graph in ("full", "segmented"), "issues " + what + " between two "
            "graphs: --hip-graph {c.hip_graph} is not supported (auto resolves to split)")


_NO_FORM = "--topology {c.topology} (no ps, sharded or two-stage form is built)"
_ONEBIT = (lambda c: c.optimizer in ("onebit_adam", "onebit_lamb"),
           "is not the sign codec: --optimizer {c.optimizer} exchanges sign-compressed momentum "
           "(--compress sign)")
_PULL = (lambda c: c.pull_compress is not None,
         "has no parameter-server form: --pull-compress belongs to --topology ps")
_EF_MODE = (lambda c: c.ef_mode != "dgc",
            "keeps a plain residual with the momentum on the receiver: --ef-mode {c.ef_mode} is "
            "not supported (leave --ef-mode unset)")


# ---- the adapters of the top-k codecs (topk and topk_qsgd share them) ------------------------------
_TOPK = dict(
    gpu_encode=lambda c, b, grad, payload, key, resid, key_tensor, dgc, apply: ops.topk_encode(
        c.dplans[b], grad, payload, c.layouts[b], c.levels, c.norm, key, resid, key_tensor,
        dgc=dgc, apply=apply),
    cpu_encode=lambda c, b, grad, key, resid, dgc, ef21: oracle.encode_topk(
        grad, c.plans[b], c.layouts[b], c.levels, c.norm, key, resid, dgc, ef21),
    gpu_decode=lambda c, b, recv, **kw: ops.topk_decode_apply(
        c.dplans[b], recv, c.layouts[b], c.levels, **kw))

_ALL = (
    Kind("none", lambda c: "none", wire_dtype=torch.float32, bits=True),
    Kind("fp16", lambda c: "fp16", wire_dtype=torch.float16, bits=True),
    Kind("bf16", lambda c: "bf16", wire_dtype=torch.bfloat16, bits=True),
    Kind("qsgd", lambda c: f"qsgd{c.bits}b(s={c.levels},{c.norm})", bits=True, levels=True,
         gpu_encode=lambda c, b, grad, payload, key, resid, key_tensor, dgc, apply:
         ops.qsgd_encode(c.dplans[b], grad, payload, c.layouts[b], c.levels, c.norm, key, resid,
                         key_tensor),
         cpu_encode=lambda c, b, grad, key, resid, dgc, ef21: oracle.encode_qsgd(
             grad, c.plans[b], c.layouts[b], c.levels, c.norm, key, resid),
         gpu_decode=lambda c, b, recv, **kw: ops.qsgd_decode_apply(
             c.dplans[b], recv, c.layouts[b], c.levels, **kw)),
    Kind("topk", lambda c: f"topk{c.ratio:g}", bits=True, density=True, **_TOPK),
    Kind("topk_qsgd", lambda c: f"topk{c.ratio:g}+qsgd{c.bits}b(s={c.levels},{c.norm})",
         bits=True, levels=True, density=True, **_TOPK),
    Kind("sign", lambda c: "sign1b-h" if c.rotate == "hadamard" else "sign1b",
         gpu_encode=lambda c, b, grad, payload, key, resid, key_tensor, dgc, apply:
         ops.sign_encode(c.dplans[b], grad, payload, c.layouts[b], resid, rot_key=c.rot_key(b)),
         cpu_encode=lambda c, b, grad, key, resid, dgc, ef21: oracle.encode_sign(
             grad, c.plans[b], c.layouts[b], resid, c.rot_key(b)),
         gpu_decode=lambda c, b, recv, **kw: ops.sign_decode_apply(
             c.dplans[b], recv, c.layouts[b], rot_key=c.rot_key(b), **kw)),
    # PowerSGD (parallel/powersgd.py): two dependent all-reduces of rank-r factors per bucket,
    # always with its residual, averaged with 1/N inside its kernels
    Kind("powersgd", lambda c: f"powersgd-r{c.rank}",
         own_exchange=OwnExchange("PowerSGD", "PowerSGD exchanges two dependent all-reduces per "
                                  "bucket"),
         flags=(Flag("powersgd_rank", "rank", 4),), ef_default=True,
         refusals=(
             (lambda c: c.powersgd_rank not in POWERSGD_RANKS,
              "supports ranks 1, 2, 4 and 8, not --powersgd-rank {c.powersgd_rank}"),
             _topology("averages its factors by all-reduce on every rank: it does not run with "
                       "--topology {c.topology}"),
             _local("exchanges every step: it does not run with --sync-every > 1"),
             _best("averages all workers: it does not run with --select-best"),
             _no_ef("is a biased compressor that relies on its residual: it does not run with "
                    "--no-error-feedback"),
             _predivide("averages its factors with 1/N in its kernels: it does not run with"),
             _one_graph("its two all-reduces, the orthogonalisation and the back-projection"),
             _ONEBIT)),
    # Distributed Lion (parallel/engine.py GradientExchange, vote mode): every rank sends the sign
    # of its own Lion update, one bit per element and no magnitude, so only Lion can step on it
    # and nothing that scales or compensates a magnitude applies
    Kind("vote", lambda c: "vote1b",
         flags=(Flag("vote_aggregate", "aggregate", "majority"),
                Flag("vote_exchange", None, "allgather")), ef_default=False,
         refusals=(
             (lambda c: c.optimizer != "lion",
              "carries no magnitudes, only Lion's sign update can step on it: it needs --optimizer "
              "lion, not {c.optimizer!r}"),
             _topology("is an all-gather of every rank's bits: it does not run with --topology "
                       "{c.topology} (the vote's own sharded form is --vote-exchange twostage)"),
             _local("votes every step: it does not run with --sync-every > 1"),
             _best("takes the vote of all workers: it does not run with --select-best"),
             _predivide("counts signs, there is nothing to pre-divide: it does not run with"),
             (lambda c: c.error_feedback,
              "sends no magnitude that a residual could compensate: it does not run with "
              "--error-feedback"))),
    # MXFP8 / MXFP4 (compress/oracle.py encode_mx): the all-gather exchange's encode and fused
    # decode, with that exchange's residual (block floating point rounds to nearest: biased)
    Kind("mx", lambda c: "mx" + c.fmt, bits=True,
         gpu_encode=lambda c, b, grad, payload, key, resid, key_tensor, dgc, apply:
         ops.mx_encode(c.dplans[b], grad, payload, c.layouts[b], resid),
         cpu_encode=lambda c, b, grad, key, resid, dgc, ef21: oracle.encode_mx(
             grad, c.plans[b], c.layouts[b], resid),
         gpu_decode=lambda c, b, recv, **kw: ops.mx_decode_apply(
             c.dplans[b], recv, c.layouts[b], **kw),
         flags=(Flag("mx_format", "fmt", "fp8"),), ef_default=True, no_ps_form=True,
         refusals=(
             (lambda c: c.mx_format not in MX_FORMATS,
              "sends fp8 or fp4 elements: --mx-format {c.mx_format!r} is neither"),
             _topology("runs the all-gather exchange, which keeps its residual: it does not run "
                       "with " + _NO_FORM),
             _local("keeps its residual in the all-gather exchange: it does not run with "
                    "--sync-every > 1"),
             _best("keeps its residual in the all-gather exchange: it does not run with "
                   "--select-best"),
             _ONEBIT, _PULL)),
    # TernGrad (compress/oracle.py encode_tern): the all-gather exchange's encode and fused decode,
    # every rank's codes decoded with its own scaler; unbiased apart from clipping, and the paper
    # runs without error feedback
    Kind("tern", lambda c: f"tern2b(c={c.clip:g})" if c.clip > 0 else "tern2b",
         gpu_encode=lambda c, b, grad, payload, key, resid, key_tensor, dgc, apply:
         ops.tern_encode(c.dplans[b], grad, payload, c.layouts[b], c.clip, key, resid,
                         key_tensor),
         cpu_encode=lambda c, b, grad, key, resid, dgc, ef21: oracle.encode_tern(
             grad, c.plans[b], c.layouts[b], c.clip, key, resid),
         gpu_decode=lambda c, b, recv, **kw: ops.tern_decode_apply(
             c.dplans[b], recv, c.layouts[b], **kw),
         flags=(Flag("tern_clip", "clip", oracle.TERN_CLIP),), ef_default=False, no_ps_form=True,
         refusals=(
             (lambda c: not float(c.tern_clip) >= 0.0,
              "clips at a multiple of the rms: --tern-clip {c.tern_clip!r} must be >= 0"),
             _topology("decodes every rank's codes with that rank's scaler in the all-gather "
                       "exchange: it does not run with " + _NO_FORM),
             _local("is built into the all-gather exchange's every-step path: it does not run "
                    "with --sync-every > 1"),
             _best("is built into the all-gather exchange's every-step path: it does not run "
                   "with --select-best"),
             _ONEBIT, _PULL)),
    # the count sketch (parallel/sketch.py): two dependent all-reduces per bucket (the table, then
    # the selected coordinates' values), always with its plain residual, averaged with 1/N in its
    # decode; k per tensor is --topk-ratio / --topk-dense-below's
    Kind("sketch", lambda c: f"sketch-r{c.rows}", density=True,
         gpu_decode=_TOPK["gpu_decode"],  # of the one summed payload (Codec.sk_decode_apply_sgd)
         own_exchange=OwnExchange("sketch", "the count sketch exchanges two dependent all-reduces "
                                  "per bucket"),
         flags=(Flag("sketch_rows", "rows", 3), Flag("sketch_width", "width", 2.0)),
         ef_default=True, no_ps_form=True, auto_graph="split",
         refusals=(
             (lambda c: c.sketch_rows not in SKETCH_ROWS,
              "takes the median of an odd number of rows: --sketch-rows must be 1, 3 or 5, not "
              "{c.sketch_rows}"),
             (lambda c: not float(c.sketch_width) > 0.0,
              "sizes its table in columns per selected element: --sketch-width must be > 0, not "
              "{c.sketch_width!r}"),
             _topology("sums its tables by all-reduce on every rank: it does not run with "
                       "--topology {c.topology}"),
             _local("exchanges every step: it does not run with --sync-every > 1"),
             _best("sums all workers' sketches: it does not run with --select-best"),
             _no_ef("sends only the heavy coordinates and relies on its residual for the rest: it "
                    "does not run with --no-error-feedback"),
             _EF_MODE,
             _predivide("averages the summed values with 1/N in its decode: it does not run with"),
             _PULL,
             _one_graph("its two all-reduces, the estimate, the selection and the gather"),
             _ONEBIT)),
    # the threshold-search sparsifier (compress/oracle.py encode_thresh): the all-gather exchange's
    # encode and fused decode with that exchange's plain residual (what lies below the threshold
    # is never sent without it); k per tensor is --topk-ratio / --topk-dense-below's.
    # --qsgd-bits / --qsgd-levels and --ef-warmup none are accepted and unused (the values travel
    # as fp32; there is no warm-up)
    Kind("thresh", lambda c: f"thresh-k{c.ratio:g}", density=True,
         gpu_encode=lambda c, b, grad, payload, key, resid, key_tensor, dgc, apply:
         ops.thresh_encode(c.dplans[b], grad, payload, c.layouts[b], resid, c.thr_state[b]),
         cpu_encode=lambda c, b, grad, key, resid, dgc, ef21: oracle.encode_thresh(
             grad, c.plans[b], c.layouts[b], resid),
         gpu_decode=lambda c, b, recv, **kw: ops.thresh_decode_apply(
             c.dplans[b], recv, c.layouts[b], **kw),
         ef_default=True, no_ps_form=True,
         refusals=(
             _topology("runs the all-gather exchange, which keeps its residual: it does not run "
                       "with " + _NO_FORM),
             _local("keeps its residual in the all-gather exchange's every-step path: it does not "
                    "run with --sync-every > 1"),
             _best("keeps its residual in the all-gather exchange's every-step path: it does not "
                   "run with --select-best"),
             _PULL, _EF_MODE, _ONEBIT)),
    # IntSGD (parallel/intsgd.py): int8 codes under one model-wide scale, summed by one all-reduce
    # per bucket; the scale follows the norm of the last SGD update.  Unbiased apart from
    # clipping: error feedback either way, off unless asked for.  --qsgd-bits / --qsgd-levels and
    # --ef-warmup none are accepted and unused (the wire is int8 with q = floor(127 / world)
    # levels; no warm-up)
    Kind("intsgd", lambda c: "intsgd8",
         own_exchange=OwnExchange("intsgd", "the wrapped optimizer owns the step, so the update "
                                  "norm IntSGD's scale follows is not visible"),
         ef_default=False, no_ps_form=True, auto_graph="split",
         refusals=(
             (lambda c: c.optimizer != "sgd",
              "ties its quantisation step to the last update's norm over lr, which is a gradient "
              "only under SGD (about 1 per element under Adam-like rules, so the step would dwarf "
              "every gradient): it needs --optimizer sgd, not {c.optimizer!r}"),
             _topology("sums its codes by all-reduce on every rank: it does not run with "
                       + _NO_FORM),
             _local("measures the update of every step for its scale: it does not run with "
                    "--sync-every > 1"),
             _best("sums all workers' codes: it does not run with --select-best"),
             _PULL,
             _predivide("averages the summed codes with 1 / (alpha N) in its decode: it does not "
                        "run with"),
             _EF_MODE,
             _one_graph("its all-reduces"))),
)
KINDS = {k.name: k for k in _ALL}

# The order in which Config.resolved() visits the kinds that have rules of their own, around its
# global error-feedback default: an earlier kind's refusal or orphan flag is the one reported, and
# the powersgd and sketch refusals follow the sign codec's and the two-stage topology's
RESOLVED_FIRST = ("mx", "tern", "thresh", "intsgd", "vote")
RESOLVED_LAST = ("powersgd", "sketch")
