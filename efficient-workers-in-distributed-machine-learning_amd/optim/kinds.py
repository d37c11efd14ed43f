"""What each optimizer is built from: one :class:`Kind` per ``--optimizer`` value.

The command line (its ``--optimizer`` choices and per-optimizer flags), ``Config.resolved()``
(the flags' defaults, their checks, orphan flags), the trainer (the keywords it hands over) and
``make_optimizer`` read this table; a new optimizer is one entry here plus its class.
"""
from dataclasses import dataclass, field
from typing import Callable, NamedTuple, Optional

from . import flat as F

# make_optimizer's common keywords -> the Config field the trainer fills each from (lr is the
# trainer's own: --lr after --lr-scale-world)
COMMON = {"momentum": "momentum", "dampening": "dampening", "weight_decay": "weight_decay",
          "nesterov": "nesterov", "eps": "adam_eps", "freeze_step": "onebit_warmup_steps",
          "betas": "lion_betas", "seed": "seed"}


class Option(NamedTuple):
    """A command-line flag that belongs to one optimizer: ``--galore-rank`` is
    ``Config.galore_rank``, ``make_optimizer``'s ``galore_rank=`` and ``FlatGalore``'s ``rank``."""
    field: str
    kw: str  # make_optimizer's keyword
    arg: str  # the constructor's argument
    type: Callable  # int | float | str | bool (a bool flag takes no value)
    default: object  # of an unset (None) flag under its optimizer
    ok: Optional[Callable] = None  # the value is admissible (with ``choices``: one of them)
    why: str = ""  # the refusal is the flag, a space and this
    choices: Optional[tuple] = None

    @property
    def flag(self) -> str:
        return "--" + self.field.replace("_", "-")

    def refuses(self, v) -> bool:
        if v is None:  # an option without a default of its own (--muon-aux-lr: --lr)
            return False
        if self.choices is not None:
            return v not in self.choices
        return self.ok is not None and not self.ok(v)


@dataclass(frozen=True)
class Kind:
    name: str
    cls: type
    common: tuple  # the constructor arguments taken from the common keywords, when given
    options: tuple = ()
    fixed: dict = field(default_factory=dict)  # constructor arguments the name itself sets
    # (condition on the keywords, reason): make_optimizer raises the reason when it holds
    refusal: Optional[tuple] = None

    def build(self, flat, kw):
        """``cls(flat, ...)`` from ``make_optimizer``'s keywords: the common ones this optimizer
        takes, its options under their keywords (None: the default), then ``fixed``."""
        if self.refusal is not None and self.refusal[0](kw):
            raise ValueError(self.refusal[1])
        args = {k: kw[k] for k in self.common if kw.get(k) is not None}
        for o in self.options:
            v = kw.get(o.kw)
            args[o.arg] = o.default if v is None else v
        return self.cls(flat, **{**args, **self.fixed})


def _rank16(r):
    return not r % 16 and 16 <= r <= 128


_SGD = ("lr", "momentum", "dampening", "weight_decay", "nesterov")
_ADAM = ("lr", "weight_decay", "eps")

_ALL = (
    Kind("sgd", F.FlatSGD, _SGD),
    Kind("adam", F.FlatAdam, _ADAM + ("amsgrad",)),
    Kind("amsgrad", F.FlatAdam, _ADAM, fixed={"amsgrad": True}),
    Kind("adam8bit", F.FlatAdam8bit, _ADAM,
         refusal=(lambda kw: kw.get("amsgrad", False),
                  "8-bit Adam has no AMSGrad: a running maximum of the second moment would be a "
                  "third quantised state")),
    Kind("onebit_adam", F.FlatOnebitAdam, _ADAM + ("amsgrad", "freeze_step")),
    Kind("lars", F.FlatLARS, _SGD, options=(
        Option("lars_eta", "eta", "eta", float, 0.001, lambda v: v > 0, "must be > 0"),)),
    Kind("lamb", F.FlatLAMB, _ADAM),
    Kind("lion", F.FlatLion, ("lr", "betas", "weight_decay")),
    Kind("onebit_lamb", F.FlatOnebitLamb, _ADAM + ("freeze_step",)),
    Kind("muon", F.FlatMuon, ("lr", "momentum", "weight_decay", "nesterov"), options=(
        Option("muon_ns_steps", "ns_steps", "ns_steps", int, 5, lambda v: 1 <= v <= 10,
               "must lie in 1..10"),
        Option("muon_ns_dtype", "ns_dtype", "ns_dtype", str, "fp32", None, "is fp32 or bf16",
               ("fp32", "bf16")),
        Option("muon_aux_lr", "aux_lr", "aux_lr", float, None, lambda v: v > 0, "must be > 0"))),
    Kind("adafactor", F.FlatAdafactor, ("lr", "weight_decay"), options=(
        Option("adafactor_beta1", "adafactor_beta1", "beta1", float, 0.0,
               lambda v: 0.0 <= v < 1.0, "must lie in [0, 1)"),
        Option("adafactor_clip", "adafactor_clip", "clip", float, 1.0, lambda v: v > 0,
               "must be > 0"),
        Option("adafactor_scale_parameter", "adafactor_scale_parameter", "scale_parameter", bool,
               False))),
    Kind("galore", F.FlatGalore, _ADAM, options=(
        Option("galore_rank", "galore_rank", "rank", int, 64, _rank16,
               "must be a multiple of 16 in 16..128"),
        Option("galore_update_gap", "galore_update_gap", "update_gap", int, 200,
               lambda v: v >= 1, "must be >= 1"),
        Option("galore_scale", "galore_scale", "scale", float, 0.25, lambda v: v > 0,
               "must be > 0"))),
    Kind("apollo", F.FlatApollo, _ADAM + ("seed",), options=(
        Option("apollo_rank", "apollo_rank", "rank", int, 64, lambda v: v == 1 or _rank16(v),
               "must be 1 or a multiple of 16 in 16..128"),
        Option("apollo_update_gap", "apollo_update_gap", "update_gap", int, 200,
               lambda v: v >= 1, "must be >= 1"),
        Option("apollo_scale", "apollo_scale", "scale", float, 1.0, lambda v: v > 0,
               "must be > 0"),
        Option("apollo_scale_type", "apollo_scale_type", "scale_type", str, "channel", None,
               "is channel or tensor", ("channel", "tensor")))),
)
# in the order Config.resolved() visits them: of two refused flags, the one that belongs to the
# earlier optimizer is the one reported
KINDS = {k.name: k for k in _ALL}
