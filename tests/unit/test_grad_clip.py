"""Global-norm gradient clipping on the CPU: the oracle (``compress/oracle.py clip_grad_norm_``)
against ``torch.nn.utils.clip_grad_norm_``, the command line's refusals and threshold, and the CPU
trainer with an inactive and an active clip."""
import json
import math

import pytest
import torch

import ewdml
from ewdml.compress import oracle
from ewdml.parallel.clip import GradClipper, clip_threshold

SIZES = [1, 63, 64, 8191, 8193, 3 * 8192 + 5]
BF16_AT = 3  # the 8191-element tensor is bf16


def _grads(zero=False):
    g = torch.Generator().manual_seed(7)
    out = []
    for i, n in enumerate(SIZES):
        t = torch.zeros(n) if zero else torch.randn(n, generator=g)
        out.append(t.bfloat16() if i == BF16_AT else t)
    return out


def _torch_clip(grads, max_norm):
    """torch's clip on parameters holding ``grads`` (bf16 as its exact fp32 values)."""
    ps = [torch.nn.Parameter(torch.zeros(g.numel())) for g in grads]
    for p, g in zip(ps, grads):
        p.grad = g.float().clone()
    norm = torch.nn.utils.clip_grad_norm_(ps, max_norm)
    return float(norm), [p.grad for p in ps]


def _bits(t):
    return t.view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32)


def test_oracle_active_matches_torch():
    grads = _grads()
    norm_ref, _ = _torch_clip(grads, 1.0)
    C = 0.25 * norm_ref
    norm_ref, want = _torch_clip(grads, C)
    before = [g.clone() for g in grads]
    norm, coef = oracle.clip_grad_norm_(grads, C)
    assert norm.dtype == coef.dtype == torch.float32 and norm.dim() == 0
    assert abs(float(norm) - norm_ref) <= 1e-6 * norm_ref
    assert abs(float(coef) - C / (norm_ref + 1e-6)) <= 1e-6 * float(coef) and float(coef) < 1
    for i, (g, w, b) in enumerate(zip(grads, want, before)):
        assert g.dtype == b.dtype
        if g.dtype == torch.bfloat16:  # the fp32 product, rounded to nearest even
            assert torch.equal(_bits(g), _bits((b.float() * coef).bfloat16())), i
        else:
            assert torch.equal(_bits(g), _bits(b * coef)), i  # one fp32 multiply
            torch.testing.assert_close(g, w, rtol=1e-6, atol=0.0, msg=str(i))
    total = math.sqrt(sum(float((g.double() ** 2).sum()) for g in grads
                          if g.dtype == torch.float32)
                      + float(((before[BF16_AT].double() * float(coef)) ** 2).sum()))
    assert abs(total - C) <= 1e-4 * C  # the clipped gradient has norm C (bf16 rounding aside)


def test_oracle_inactive_is_bitwise_and_zero_gradient():
    grads = _grads()
    before = [g.clone() for g in grads]
    norm, coef = oracle.clip_grad_norm_(grads, 1e9)
    assert float(coef) == 1.0 and float(norm) > 0
    for g, b in zip(grads, before):
        assert torch.equal(_bits(g), _bits(b))
    zeros = _grads(zero=True)
    norm, coef = oracle.clip_grad_norm_(zeros, 0.5)
    assert float(norm) == 0.0 and float(coef) == 1.0
    assert all(bool((z == 0).all()) for z in zeros)
    with pytest.raises(ValueError, match="max_norm must be > 0"):
        oracle.clip_grad_norm_(_grads(), 0.0)


BASE = ["--network", "LeNet", "--dataset", "MNIST", "--batch-size", "16", "--synthetic-size",
        "256", "--eval-freq", "0", "--quiet", "--device", "cpu", "--no-legacy-ckpt",
        "--log-interval", "1"]
CLIP = ["--clip-grad-norm", "1.0"]


def test_cli_fields_and_threshold():
    c = ewdml.parse_args(BASE)
    assert c.clip_grad_norm is None and c.clip_scale_world is False
    c = ewdml.parse_args(BASE + ["--clip-grad-norm", "2.5", "--clip-scale-world"])
    assert c.clip_grad_norm == 2.5 and c.clip_scale_world is True
    assert ewdml.Config(clip_grad_norm=0.5).resolved().clip_grad_norm == 0.5
    assert clip_threshold(3.0, 4, False) == 3.0
    assert clip_threshold(3.0, 4, True) == 1.5  # C / sqrt(4)
    assert clip_threshold(3.0, 1, True) == 3.0
    for extra in (["--compress", "none"], ["--compress", "sign"], ["--compress", "powersgd"],
                  ["--compress", "sign", "--topology", "twostage"],
                  ["--compress", "sign", "--optimizer", "onebit_adam", "--onebit-warmup-steps",
                   "2"], ["--hip-graph", "full"], ["--hip-graph", "off"]):
        ewdml.parse_args(BASE + CLIP + extra)


@pytest.mark.parametrize("extra,why", [
    (["--clip-grad-norm", "0"], "must be > 0"),
    (["--clip-grad-norm", "-1"], "must be > 0"),
    (["--clip-scale-world"], "needs --clip-grad-norm"),
    (CLIP + ["--topology", "ps"], "--topology ps is out of scope"),
    (CLIP + ["--topology", "sharded"], "--topology sharded is out of scope"),
    (CLIP + ["--method", "1"], "--topology ps is out of scope"),
    (CLIP + ["--sync-every", "4"], r"local steps \(--sync-every > 1\) are out of scope"),
    (CLIP + ["--select-best"], "--select-best is out of scope"),
    (CLIP + ["--hip-graph", "segmented"], "nothing to overlap"),
])
def test_refusals_say_why(extra, why):
    with pytest.raises(ValueError, match=why) as e:
        ewdml.parse_args(BASE + extra)
    assert "--clip-" in str(e.value)


def test_producer_stage_is_refused_by_the_trainer(monkeypatch):
    from ewdml.runtime import Trainer

    monkeypatch.setenv("EWDML_PRODUCER_STAGE", "1")
    with pytest.raises(ValueError, match="EWDML_PRODUCER_STAGE=1 .* never stores it"):
        Trainer(ewdml.parse_args(BASE + CLIP))


def test_auto_graph_plan_never_segments_with_a_clip():
    from ewdml.parallel.engine import plan_graph_mode

    kw = dict(world=8, comm_kind="rccl-stream", codec_kind="none", grad_numel=25_000_000)
    assert plan_graph_mode(**kw)["mode"] == "segmented"
    got = plan_graph_mode(clip=True, **kw)
    assert got["mode"] == "full" and "--clip-grad-norm" in got["reason"]
    assert plan_graph_mode(overlap=False, **kw)["mode"] == "full"


def test_clipper_scales_world_and_skips_padding():
    from ewdml.parallel.flat import FlatModel

    ps = [torch.nn.Parameter(torch.zeros(n)) for n in (5, 70, 8193)]
    flat = FlatModel(ps, bucket_bytes=1024)
    assert len(flat.buckets) > 1
    flat.grad.fill_(float("nan"))  # the alignment padding stays NaN and is never read
    g = torch.Generator().manual_seed(3)
    for p in ps:
        p.grad.copy_(torch.randn(p.numel(), generator=g))
    ref = math.sqrt(sum(float((p.grad.double() ** 2).sum()) for p in ps))
    before = flat.grad.clone()
    clip = GradClipper(flat, 2.0, world=4, scale_world=True)
    assert clip.max_norm == 1.0 and clip.last() is None
    clip.run()
    norm, coef = clip.last()
    assert abs(norm - ref) <= 1e-6 * ref and abs(coef - 1.0 / (ref + 1e-6)) <= 1e-6 * coef
    for p, o in zip(flat.params, flat.offsets):
        n = p.numel()
        want = before[o:o + n] * torch.tensor(coef, dtype=torch.float32)
        assert torch.equal(flat.grad[o:o + n].view(torch.int32), want.view(torch.int32))
    pad = torch.ones(flat.numel, dtype=torch.bool)
    for p, o in zip(flat.params, flat.offsets):
        pad[o:o + p.numel()] = False
    assert bool(pad.any()) and bool(flat.grad[pad].isnan().all())
    assert torch.equal(flat.grad[pad].view(torch.int32), before[pad].view(torch.int32))


SGD = BASE + ["--compress", "none", "--momentum", "0", "--lr", "0.05"]


def _train(tmp_path, name, extra, steps):
    from ewdml.runtime import Trainer

    mf = tmp_path / f"{name}.jsonl"
    tr = Trainer(ewdml.parse_args(SGD + extra + ["--max-steps", str(steps), "--train-dir",
                                                 str(tmp_path / name), "--metrics-file", str(mf)]))
    p0 = tr.flat.data.clone()
    tr.fit()
    recs = [json.loads(line) for line in (tmp_path / f"{name}.rank0.jsonl").read_text().splitlines()
            if line.strip()]
    return p0, tr.flat.data.clone(), [r for r in recs if "step" in r and "loss" in r]


def test_trainer_inactive_clip_is_bitwise(tmp_path):
    _, plain, recs0 = _train(tmp_path, "plain", [], 3)
    _, clipped, recs = _train(tmp_path, "clip", ["--clip-grad-norm", "1e9"], 3)
    assert torch.equal(plain.view(torch.int32), clipped.view(torch.int32))
    assert all("grad_norm" not in r for r in recs0)
    assert len(recs) == 3 and all(r["clip_coef"] == 1.0 and r["grad_norm"] > 0 for r in recs)


def test_trainer_active_clip_moves_by_lr_times_c(tmp_path):
    _, _, recs = _train(tmp_path, "probe", ["--clip-grad-norm", "1e9"], 1)
    norm1 = recs[0]["grad_norm"]
    C = 0.5 * norm1  # below the first step's norm: active
    p0, p1, recs = _train(tmp_path, "active", ["--clip-grad-norm", repr(C)], 1)
    assert recs[0]["clip_coef"] < 1 and recs[0]["grad_norm"] == norm1
    moved = float((p1.double() - p0.double()).norm())
    print(f"norm {norm1:.6f} C {C:.6f} |dp| {moved:.9f} lr*C {0.05 * C:.9f}")
    assert abs(moved - 0.05 * C) <= 1e-5 * 0.05 * C
