"""The argument structs of ``ops/csrc/ewdml_ops.h`` as Python sees them (``ops/csrc/bindings.cpp``):
every field of the header is bound under its own name and type, a new object is all zero,
``ops._args`` fills by name, and the entry points that refuse an empty bucket do so for default
arguments before any HIP call.  Needs the built extension and no device."""
import os
import re

import numpy as np
import pytest

from ewdml import ops

pytestmark = pytest.mark.skipif(not ops.available(), reason="the extension is not built")

HEADER = os.path.join(os.path.dirname(ops.__file__), "csrc", "ewdml_ops.h")
BOUND = ["TopkEncodeArgs", "TopkDecodeArgs", "QsgdEncodeArgs", "QsgdDecodeArgs", "SignEncodeArgs",
         "SignReduceArgs", "SignOnebitArgs", "SignLambArgs", "SignDecodeArgs", "MxEncodeArgs",
         "MxDecodeArgs", "TernEncodeArgs", "TernDecodeArgs", "PsgdArgs", "SgdFlatArgs",
         "AdamFlatArgs", "LionFlatArgs", "LionEncodeArgs", "LionVoteArgs", "VoteReduceArgs",
         "LayerwiseArgs", "ClipArgs", "OuterArgs", "StepArgs"]
WITH_STEP = ["TopkDecodeArgs", "QsgdDecodeArgs", "SignDecodeArgs", "MxDecodeArgs",
             "TernDecodeArgs", "PsgdArgs"]
# a value each C type holds exactly and a narrower one would not
VALUES = {"uintptr_t": 0x7FFF123456789AB0, "int": -123456, "uint32_t": 0xFFFFFFFF,
          "float": 0.15625, "double": 0.1, "long long": (1 << 40) + 3}
STEP_DEFAULTS = dict(param=0, mom=0, grad_out=0, shadow=0, lr=0.0, momentum=0.0, dampening=0.0,
                     weight_decay=0.0, grad_scale=1.0, nesterov=0, first=0, apply=0, key_state=0,
                     key_seed=0, key_rank=0, lr_ptr=0)


def _header_fields():
    """{struct: {field: C type}} of the header, GradSrc members left out."""
    text = re.sub(r"//[^\n]*", "", open(HEADER).read())
    out = {}
    for name, body in re.findall(r"struct (\w+) \{(.*?)\n\};", text, re.S):
        fields = {}
        for decl in body.split(";"):
            m = re.fullmatch(r"\s*(const \w+\*|long long|\w+)\s+(.+?)\s*", decl, re.S)
            if m and m.group(1) != "GradSrc":
                for f in m.group(2).split(","):
                    fields[f.strip()] = m.group(1)
        out[name] = fields
    return out


FIELDS = _header_fields()


def _bound(cls):
    return sorted(n for n, v in vars(cls).items() if isinstance(v, property))


def _same(a, b):
    return type(a) is type(b) and a == b


def _is_default_step(s):
    return all(_same(getattr(s, f), v) for f, v in STEP_DEFAULTS.items())


@pytest.mark.parametrize("name", BOUND)
def test_every_header_field_is_bound_and_a_new_object_is_zero(name):
    C = ops.require()
    cls = getattr(C, name)
    assert _bound(cls) == sorted(FIELDS[name]) and "src" not in _bound(cls)
    a = cls()
    assert not hasattr(a, "src")
    for f, ctype in FIELDS[name].items():
        v = getattr(a, f)
        if ctype == "StepArgs":
            assert name in WITH_STEP and f == "step" and _is_default_step(v)
        elif name == "StepArgs":
            assert _same(v, STEP_DEFAULTS[f]), f
        else:
            assert _same(v, 0.0 if ctype in ("float", "double") else 0), f
    assert ("step" in FIELDS[name] and FIELDS[name]["step"] == "StepArgs") == (name in WITH_STEP)


@pytest.mark.parametrize("name", BOUND)
def test_every_field_round_trips_a_value_of_its_type(name):
    C = ops.require()
    a = getattr(C, name)()
    for f, ctype in FIELDS[name].items():
        if ctype == "StepArgs":
            a.step = C.StepArgs(grad_out=64, lr=0.5, key_seed=7)
            assert (a.step.grad_out, a.step.lr, a.step.key_seed) == (64, 0.5, 7)
            assert a.step.grad_scale == 1.0 and a.step.apply == 0
            continue
        setattr(a, f, VALUES[ctype])
        assert _same(getattr(a, f), VALUES[ctype]), f
        if ctype == "uint32_t":
            for bad in (-1, 1 << 32):
                with pytest.raises(TypeError):
                    setattr(a, f, bad)
            assert getattr(a, f) == VALUES[ctype]
        if ctype == "float":  # a double that fp32 does not hold is rounded as C's (float) does
            setattr(a, f, 0.1)
            assert getattr(a, f) == float(np.float32(0.1)) != 0.1
    for f, ctype in FIELDS[name].items():  # no field's store reached another
        if ctype == "float":
            assert getattr(a, f) == float(np.float32(0.1)), f
        elif ctype != "StepArgs":
            assert getattr(a, f) == VALUES[ctype], f


def test_args_fills_by_name_and_refuses_an_unknown_field():
    C = ops.require()
    a = ops._args(C.OuterArgs, n=5, lr=0.25, anchor=1 << 40)
    assert (a.n, a.lr, a.anchor, a.mu, a.stats) == (5, 0.25, 1 << 40, 0.0, 0)
    for name in BOUND:
        with pytest.raises(AttributeError):
            ops._args(getattr(C, name), no_such_field=1)
        with pytest.raises(AttributeError):
            ops._args(getattr(C, name), src=0)
    with pytest.raises(AttributeError):  # a field of another struct
        ops._args(C.TopkDecodeArgs, num_tensors=1)


def test_the_values_the_wrappers_compute():
    C = ops.require()
    a = ops._layerwise_args(C, (0.9, 0.999), 3, kind=1)
    for got, beta in ((a.beta1, 0.9), (a.beta2, 0.999)):
        assert np.float32(got).tobytes() == np.float32(beta).tobytes() and got == float(
            np.float32(beta))
    assert (a.beta1d, a.beta2d, a.kind) == (0.9, 0.999, 1)
    assert a.bc1 == float(np.float32(1.0 - 0.9 ** 3)) and a.bc2 == float(
        np.float32(1.0 - 0.999 ** 3))
    adam = ops._adam_args(C, n=8)
    assert _same(adam.bc2_sqrt, 1.0) and adam.n == 8
    assert ops._apply_args(None, None, "max") == {}


# the entry points whose first host statement refuses an empty bucket or range (a chunk, rank or
# element count of zero); the others check later, or reach the HIP runtime, and are not called
REFUSE_EMPTY = [("sign_encode", "SignEncodeArgs", True), ("mx_encode", "MxEncodeArgs", True),
                ("tern_encode", "TernEncodeArgs", True), ("lion_encode", "LionEncodeArgs", True),
                ("clip_norm", "ClipArgs", True), ("clip_scale", "ClipArgs", True),
                ("sign_decode_apply", "SignDecodeArgs", False),
                ("mx_decode_apply", "MxDecodeArgs", False),
                ("tern_decode_apply", "TernDecodeArgs", False),
                ("sign_decode_onebit", "SignOnebitArgs", False),
                ("sign_reduce_encode", "SignReduceArgs", False),
                ("sign_decode_lamb_stage", "SignLambArgs", False),
                ("lamb_onebit_apply", "SignLambArgs", False),
                ("vote_reduce", "VoteReduceArgs", False),
                ("lion_vote_apply", "LionVoteArgs", False), ("lion_flat", "LionFlatArgs", False),
                ("outer_apply", "OuterArgs", False)]


@pytest.mark.parametrize("entry,cls,grads", REFUSE_EMPTY, ids=[e[0] for e in REFUSE_EMPTY])
def test_default_arguments_are_refused_before_any_launch(entry, cls, grads):
    C = ops.require()
    a = getattr(C, cls)()
    with pytest.raises(RuntimeError, match="empty|nothing to|missing operand|the step needs"):
        getattr(C, entry)(a, [], []) if grads else getattr(C, entry)(a)


def test_the_op_selectors_are_gone():
    C = ops.require()
    for name in ("psgd", "onebit_lamb", "layerwise", "clip", "sign_encode_momentum"):
        assert not hasattr(C, name)
