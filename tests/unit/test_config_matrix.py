"""The command line's cross product of codec kinds and what they run with, against a recording.

``config_matrix.json`` (beside this file) holds, for every case of :func:`cases`, either the text
of the refusal or the resolved fields that differ from ``Config()``; each distinct outcome is
stored once and the cases, in the order of :func:`cases`, refer to it by index.  It was recorded by
:func:`resolve_all` before the per-kind blocks of ``Config.resolved()`` became one table
(``compress/kinds.py``), so a difference is a change of behaviour: a command line that resolves
to another ``Config``, is refused where it ran (or the reverse), or is refused in other words.

Record again (only when the behaviour is meant to change): ``python -m tests.unit.test_config_matrix``
"""
import dataclasses
import itertools
import json
import os

import pytest

from ewdml.config import Config, parse_args

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "config_matrix.json")

KINDS = ("none", "fp16", "bf16", "qsgd", "topk", "topk_qsgd", "sign", "powersgd", "vote", "mx",
         "tern", "sketch", "thresh", "intsgd")
TOPOLOGIES = ("allgather", "ps", "sharded", "twostage")
OPTIMIZERS = ("sgd", "adam", "lion", "onebit_adam", "onebit_lamb")
EXTRA_FLAGS = (
    "--pull-compress qsgd", "--predivide 2", "--ef-mode plain", "--ef-mode ef21",
    "--hip-graph full", "--hip-graph segmented", "--hip-graph split", "--error-feedback",
    "--no-error-feedback", "--sign-rotate hadamard", "--mx-format fp4", "--tern-clip 1",
    "--sketch-rows 5", "--sketch-width 1", "--powersgd-rank 2", "--vote-aggregate average",
    "--vote-exchange twostage", "--clip-grad-norm 1")


def cases():
    """(name, thunk) of every case; the name is the argv (or the constructor call) as one string.
    --device cpu everywhere: the ef21 rule then does not ask whether the machine has a GPU."""
    out = []

    def cli(*words):
        argv = " ".join(("--device cpu",) + words).split()
        out.append((" ".join(argv), lambda: parse_args(argv)))

    for kind, topo, every, best, opt in itertools.product(KINDS, TOPOLOGIES, (1, 4), (False, True),
                                                          OPTIMIZERS):
        cli(f"--compress {kind} --topology {topo} --sync-every {every}",
            "--select-best" if best else "", f"--optimizer {opt}",
            "--onebit-warmup-steps 2" if opt.startswith("onebit") else "")
    for kind, opt, flag in itertools.product(KINDS, ("sgd", "lion"), EXTRA_FLAGS):
        cli(f"--compress {kind} --optimizer {opt}", flag)
    for kind in KINDS:
        out.append((f"Config(device='cpu', topology='ps', compress='qsgd', pull_compress={kind!r})",
                    lambda kind=kind: Config(device="cpu", topology="ps", compress="qsgd",
                                             pull_compress=kind).resolved()))
    return out


def resolve_all() -> dict:
    """Every case resolved now: ``outcomes`` (each distinct one once: the text of a refusal, or
    the dict of the resolved fields that differ from ``Config()``) and ``cases`` (per case, in
    order, its index into ``outcomes``)."""
    default = dataclasses.asdict(Config())
    outcomes, table = [], []
    for _, thunk in cases():
        try:
            got = dataclasses.asdict(thunk())
        except ValueError as e:
            res = str(e)
        else:  # through JSON: tuples become lists, as in the recording
            res = json.loads(json.dumps({k: v for k, v in got.items() if v != default[k]}))
        if res not in outcomes:
            outcomes.append(res)
        table.append(outcomes.index(res))
    return {"outcomes": outcomes, "cases": table}


def test_kinds_are_the_codecs():
    from ewdml.compress import codecs

    assert codecs.KINDS == KINDS


def test_config_matrix_matches_the_recording():
    with open(FIXTURE, encoding="utf-8") as f:
        want = json.load(f)
    got = resolve_all()
    assert len(got["cases"]) == len(want["cases"]), "the matrix itself changed: record again"
    diff = [(name, want["outcomes"][w], got["outcomes"][g])
            for (name, _), w, g in zip(cases(), want["cases"], got["cases"])
            if want["outcomes"][w] != got["outcomes"][g]]
    if diff:
        pytest.fail(f"{len(diff)} of {len(want['cases'])} cases differ from the recording; the "
                    "first ones:\n" + "\n".join(f"  {n}\n    recorded: {w!r}\n    now:      {g!r}"
                                                for n, w, g in diff[:10]))


if __name__ == "__main__":
    rec = resolve_all()
    with open(FIXTURE, "w", encoding="utf-8") as f:
        f.write('{"outcomes": [\n' + ",\n".join(json.dumps(o) for o in rec["outcomes"])
                + '\n],\n"cases": ' + json.dumps(rec["cases"], separators=(",", ":")) + "}\n")
    refused = sum(isinstance(rec["outcomes"][i], str) for i in rec["cases"])
    print(f"{len(rec['cases'])} cases ({refused} refused), {len(rec['outcomes'])} distinct outcomes "
          f"-> {FIXTURE}")
