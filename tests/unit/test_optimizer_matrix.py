"""The command line's cross product of optimizers and their own flags, against a recording.

``optimizer_matrix.json`` (beside this file) holds, for every case of :func:`cases`, either the
text of the refusal or the resolved fields that differ from ``Config()``; each distinct outcome is
stored once and the cases, in the order of :func:`cases`, refer to it by index.  It was recorded by
:func:`resolve_all` before the per-optimizer blocks of ``Config.resolved()`` became one table
(``optim/kinds.py``), so a difference is a change of behaviour: a command line that resolves to
another ``Config``, is refused where it ran (or the reverse), is refused in other words, or whose
two faults are reported in the other order.

Record again (only when the behaviour is meant to change):
``python -m tests.unit.test_optimizer_matrix``
"""
import dataclasses
import itertools
import json
import os

import pytest

from ewdml.config import Config, parse_args

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "optimizer_matrix.json")

OPTIMIZERS = ("sgd", "adam", "amsgrad", "adam8bit", "onebit_adam", "lars", "lamb", "lion",
              "onebit_lamb", "muon", "adafactor", "galore", "apollo")
# what the two 1-bit optimizers need to get past their own exchange rules, so that a foreign flag
# reaches its "belongs to"
ONEBIT = "--compress sign --onebit-warmup-steps 2"
# per owner: its flags, each at one valid value and then at every value its checks tell apart
# (a value outside an argparse ``choices`` list never reaches Config.resolved())
FLAGS = {
    "lars": ("--lars-eta 0.01", "--lars-eta 0", "--lars-eta -1"),
    "muon": ("--muon-ns-steps 3", "--muon-ns-steps 0", "--muon-ns-steps 11",
             "--muon-ns-dtype bf16", "--muon-ns-dtype fp32", "--muon-aux-lr 0.1",
             "--muon-aux-lr 0"),
    "adafactor": ("--adafactor-beta1 0.9", "--adafactor-beta1 0", "--adafactor-beta1 1",
                  "--adafactor-beta1 -0.1", "--adafactor-clip 2", "--adafactor-clip 0",
                  "--adafactor-scale-parameter"),
    "galore": ("--galore-rank 32", "--galore-rank 24", "--galore-rank 144", "--galore-rank 0",
               "--galore-update-gap 3", "--galore-update-gap 0", "--galore-scale 0.5",
               "--galore-scale 0"),
    "apollo": ("--apollo-rank 16", "--apollo-rank 1", "--apollo-rank 8", "--apollo-rank 24",
               "--apollo-rank 144", "--apollo-update-gap 3", "--apollo-update-gap 0",
               "--apollo-scale 2", "--apollo-scale 0", "--apollo-scale-type tensor",
               "--apollo-scale-type channel"),
    "lion": ("--lion-betas 0.8,0.9", "--lion-betas 0.9", "--lion-betas 0.9,1",
             "--lion-betas 0.9,0.99,0.999", "--lion-betas a,b"),
}
# one refused value per owner (a flag that is wrong under its own optimizer and an orphan under
# every other): each pair under every optimizer pins which of two refusals is the one reported
BAD = ("--lars-eta 0", "--muon-ns-steps 0", "--adafactor-beta1 1", "--galore-rank 24",
       "--apollo-rank 8", "--lion-betas 0.9")


def cases():
    """(name, thunk) of every case; the name is the argv as one string.  --device cpu
    everywhere, as in test_config_matrix."""
    out = []

    def cli(*words):
        argv = " ".join(("--device cpu",) + words).split()
        out.append((" ".join(argv), lambda: parse_args(argv)))

    def both(opt, *words):  # a 1-bit optimizer also with what its exchange rules ask for
        cli(f"--optimizer {opt}", *words)
        if opt.startswith("onebit"):
            cli(f"--optimizer {opt}", ONEBIT, *words)

    for opt in OPTIMIZERS:
        both(opt)
    for opt, flag in itertools.product(OPTIMIZERS, itertools.chain.from_iterable(FLAGS.values())):
        both(opt, flag)
    for opt, (a, b) in itertools.product(OPTIMIZERS, itertools.combinations(BAD, 2)):
        both(opt, a, b)
        both(opt, b, a)
    for opt, n in itertools.product(OPTIMIZERS, (2, 0)):
        cli(f"--optimizer {opt} --onebit-warmup-steps {n}")
        cli(f"--optimizer {opt} --compress sign --onebit-warmup-steps {n}")
    return out


def resolve_all() -> dict:
    """Every case resolved now, in test_config_matrix's format: ``outcomes`` (each distinct one
    once: the text of a refusal, or the dict of the resolved fields that differ from
    ``Config()``) and ``cases`` (per case, in order, its index into ``outcomes``)."""
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


def test_the_parser_offers_these_optimizers():
    from ewdml.config import build_parser

    choices = next(a.choices for a in build_parser()._actions if a.dest == "optimizer")
    assert sorted(choices) == sorted(OPTIMIZERS)


def test_optimizer_matrix_matches_the_recording():
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
