"""LARS and LAMB on the CPU: the torch oracle (compress/oracle.py lars_apply / lamb_apply) through
``FlatLARS`` / ``FlatLAMB`` against an independent per-tensor float64 implementation, the rules
that fix the trust ratio at 1, the flat buffer's padding, the state dict and the command line."""
import pytest
import torch

import ewdml
from ewdml.optim import FlatLAMB, FlatLARS, make_optimizer

from tests.layerwise_ref import (assert_state_close, make_flat, make_grad, make_pair,
                                 padding_is_zero, split)

BASE = ["--network", "LeNet", "--dataset", "MNIST", "--batch-size", "16", "--synthetic-size",
        "256", "--eval-freq", "0", "--quiet", "--device", "cpu", "--log-interval", "1000"]

CASES = [("lamb", dict(lr=0.01)),
         ("lars", dict(lr=0.1, momentum=0.9, dampening=0.1)),
         ("lars", dict(lr=0.1, momentum=0.9, nesterov=True)),
         ("lars", dict(lr=0.1))]


def _run(kind, kw, wd, steps=3, bucket_bytes=8 << 20, per_bucket=False, grad_scale=1.0):
    flat = make_flat(bucket_bytes=bucket_bytes)
    opt, ref = make_pair(kind, flat, weight_decay=wd, **kw)
    ratios = []
    for s in range(steps):
        g = make_grad(flat, s)
        if per_bucket:
            for b in flat.buckets:
                opt.step_range(b.start, b.length, g[b.start:b.start + b.length], grad_scale)
            opt.end_step()
        else:
            opt.step(grad=g, grad_scale=grad_scale)
        ref.step(split(flat, g), grad_scale)
        ratios.append((opt.ratio.clone(), list(ref.ratios)))
    return flat, opt, ref, ratios


@pytest.mark.parametrize("wd", [0.0, 1e-2])
@pytest.mark.parametrize("kind,kw", CASES)
def test_oracle_matches_float64(kind, kw, wd):
    flat, opt, ref, ratios = _run(kind, kw, wd, grad_scale=0.5)
    # the project's own tolerance for Adam (test_sgd_and_adam_flat)
    assert_state_close(flat, opt, ref, rtol=1e-5, atol=1e-6)
    for got, want in ratios:
        torch.testing.assert_close(got.double(), torch.tensor(want, dtype=torch.float64),
                                   rtol=1e-5, atol=0)
        assert float(got[0]) == 1.0  # the 1-D tensor never adapts
        assert all(float(r) != 1.0 for r in got[1:])
    assert opt.steps == 3
    mats = [opt.exp_avg, opt.exp_avg_sq] if kind == "lamb" else [opt.mom]
    assert padding_is_zero(flat, flat.data, *mats)


@pytest.mark.parametrize("kind,kw", CASES[:2])
def test_per_bucket_steps_equal_the_whole_model_step(kind, kw):
    a, _, _, ra = _run(kind, kw, 1e-2)
    b, _, _, rb = _run(kind, kw, 1e-2, bucket_bytes=4 * 8192, per_bucket=True)
    assert len(b.buckets) >= 2
    assert torch.equal(a.data.view(torch.int32), b.data.view(torch.int32))
    assert torch.equal(ra[-1][0], rb[-1][0])


@pytest.mark.parametrize("kind", ["lars", "lamb"])
def test_zero_norms_and_vectors_take_ratio_one(kind):
    flat = make_flat()
    o, n = flat.offsets[2], flat.params[2].numel()
    flat.data[o:o + n] = 0.0  # an all-zero matrix
    opt, ref = make_pair(kind, flat, lr=0.05, weight_decay=1e-2)
    g = make_grad(flat, 0)
    o4, n4 = flat.offsets[4], flat.params[4].numel()
    g[o4:o4 + n4] = 0.0  # a matrix whose gradient is zero
    opt.step(grad=g)
    ref.step(split(flat, g))
    assert float(opt.ratio[0]) == 1.0 and float(opt.ratio[2]) == 1.0
    assert float(opt.ratio[1]) != 1.0 and float(opt.ratio[3]) != 1.0
    if kind == "lars":
        assert float(opt.ratio[4]) == 1.0  # zero gradient
    assert_state_close(flat, opt, ref)
    assert padding_is_zero(flat, flat.data)
    lo, hi = opt.trust_ratio_range()
    adapting = opt.ratio[1:]
    assert lo == float(adapting.min()) and hi == float(adapting.max())


def test_a_range_that_is_no_bucket_is_refused():
    flat = make_flat()
    opt = FlatLAMB(flat)
    with pytest.raises(ValueError, match="a bucket or the whole model"):
        opt.step_range(0, 64, flat.grad[:64])


@pytest.mark.parametrize("kind,kw", CASES[:2])
def test_state_dict_round_trip(kind, kw):
    flat, opt, _, _ = _run(kind, kw, 1e-2, steps=2)
    sd = {k: (v.clone() if torch.is_tensor(v) else v) for k, v in opt.state_dict().items()}
    assert sd["kind"] == kind and sd["steps"] == 2
    g = make_grad(flat, 7)
    opt.step(grad=g)
    flat2 = make_flat()
    opt2 = make_optimizer(kind, flat2, lr=123.0)
    opt2.load_state_dict(sd)
    assert opt2.steps == 2 and opt2.lr == opt.lr
    # the parameters travel in the model's checkpoint: take them from before the third step
    flat3, _, _, _ = _run(kind, kw, 1e-2, steps=2)
    flat2.data.copy_(flat3.data)
    opt2.step(grad=g)
    assert torch.equal(flat2.data.view(torch.int32), flat.data.view(torch.int32))
    assert torch.equal(opt2.ratio, opt.ratio)


def test_make_optimizer_and_exports():
    flat = make_flat()
    a = make_optimizer("lars", flat, lr=0.1, momentum=0.9, eta=0.01, eps=1e-6, freeze_step=None)
    assert isinstance(a, FlatLARS) and a.eta == 0.01 and a.momentum == 0.9 and not a.fusable
    b = make_optimizer("lamb", flat, lr=0.002, eps=1e-6, momentum=0.9, weight_decay=0.1)
    assert isinstance(b, FlatLAMB) and b.eps == 1e-6 and b.betas == (0.9, 0.999) and not b.fusable
    assert b.weight_decay == 0.1 and b.lr == 0.002
    with pytest.raises(ValueError, match="Nesterov"):
        FlatLARS(flat, nesterov=True)


def test_cli_choices_and_lars_eta():
    c = ewdml.parse_args(BASE + ["--optimizer", "lars"])
    assert c.optimizer == "lars" and c.lars_eta == 0.001
    c = ewdml.parse_args(BASE + ["--optimizer", "lars", "--lars-eta", "0.02", "--momentum", "0.9",
                                 "--nesterov"])
    assert c.lars_eta == 0.02 and c.nesterov
    c = ewdml.parse_args(BASE + ["--optimizer", "lamb", "--adam-eps", "1e-6", "--compress", "sign"])
    assert c.optimizer == "lamb" and c.adam_eps == 1e-6 and c.error_feedback
    for opt in ("sgd", "adam", "lamb"):
        with pytest.raises(ValueError, match="--lars-eta belongs to --optimizer lars"):
            ewdml.parse_args(BASE + ["--optimizer", opt, "--lars-eta", "0.01"])
    with pytest.raises(ValueError, match="--lars-eta must be > 0"):
        ewdml.parse_args(BASE + ["--optimizer", "lars", "--lars-eta", "0"])


@pytest.mark.parametrize("opt", ["lars", "lamb"])
def test_accepted_and_refused_where_adam_is(opt):
    """Every option pair below resolves (or raises) for lars / lamb exactly as for adam."""
    for extra in (["--compress", "sign"], ["--compress", "powersgd"],
                  ["--compress", "sign", "--topology", "twostage"],
                  ["--topology", "ps"], ["--topology", "sharded"], ["--sync-every", "4"],
                  ["--compress", "topk_qsgd"], ["--compress", "sign", "--topology", "ps"],
                  ["--onebit-warmup-steps", "3"], ["--powersgd-rank", "2"]):
        outcome = []
        for o in ("adam", opt):
            try:
                ewdml.parse_args(BASE + ["--optimizer", o] + extra)
                outcome.append("ok")
            except ValueError as e:
                outcome.append(str(e))
        assert outcome[0] == outcome[1], extra


def test_trainer_logs_the_trust_ratios(tmp_path):
    import json

    from ewdml.runtime import Trainer

    mf = tmp_path / "m.jsonl"
    tr = Trainer(ewdml.parse_args(BASE[:-1] + ["1", "--optimizer", "lamb", "--lr", "0.001",
                                               "--max-steps", "2", "--train-dir", str(tmp_path),
                                               "--metrics-file", str(mf), "--no-legacy-ckpt"]))
    tr.fit()
    tr.close()
    text = (tmp_path / "m.rank0.jsonl").read_text()  # the logger's per-rank file
    recs = [json.loads(line) for line in text.splitlines() if line.strip()]
    steps = [r for r in recs if "trust_ratio_min" in r]
    assert steps and all(0 < r["trust_ratio_min"] <= r["trust_ratio_max"] for r in steps)
    lo, hi = tr.opt.trust_ratio_range()
    assert steps[-1]["trust_ratio_min"] == lo and steps[-1]["trust_ratio_max"] == hi
