"""1-bit LAMB through the trainer on CPU/Gloo: 2 and 3 ranks train LeNet for T_w = 3 dense LAMB
steps and 4 compressed-stage steps; replicas and the shared optimizer state stay bitwise identical,
the variance is frozen, the log records show the payload drop to the sign layouts and the trust
ratios in both stages, and a checkpoint taken inside the compressed stage resumes bit for bit."""
import json

import pytest
import torch

from .helpers import run_world

pytestmark = pytest.mark.slow

TW, STEPS = 3, 7
BASE = ["--network", "LeNet", "--dataset", "MNIST", "--batch-size", "16", "--synthetic-size",
        "512", "--lr", "0.002", "--eval-freq", "0", "--quiet", "--device", "cpu",
        "--log-interval", "1", "--compress", "sign", "--optimizer", "onebit_lamb",
        "--onebit-warmup-steps", str(TW), "--no-legacy-ckpt", "--weight-decay", "0.0005",
        "--bucket-mb", "0.25"]
STATE = ("exp_avg", "exp_avg_sq", "exp_avg_sq_fresh", "coeff_ema", "r_frozen", "_factors", "ratio")


def _state(tr):
    out = {name: getattr(tr.opt, name).clone() for name in STATE}
    out.update(params=tr.flat.data.clone(), resid=tr.exchange.resid.clone())
    return out


def _train(rank, world, ckpt_dir, stop_at, resume):
    """Steps up to ``stop_at`` (checkpoint there), or -- ``resume`` -- from the checkpoint on."""
    import os

    import ewdml
    from ewdml.runtime import Trainer

    args = BASE + ["--max-steps", str(stop_at), "--train-dir", ckpt_dir, "--metrics-file",
                   os.path.join(ckpt_dir, f"m{int(resume)}.jsonl")]
    tr = Trainer(ewdml.parse_args(args + (["--resume"] if resume else [])))
    out = {"start": tr.step, "buckets": len(tr.flat.buckets)}
    kinds = []
    orig = tr.train_step

    def step(*a, **kw):
        r = orig(*a, **kw)
        kinds.append(tr.exchange.codec.kind)
        if tr.step == TW:
            out["v_at_tw"] = tr.opt.exp_avg_sq.clone()
        return r

    tr.train_step = step
    tr.fit()
    out["kinds"] = kinds
    out["layout_bytes"] = sum(lay.nbytes for lay in tr.exchange.codec.layouts)
    out["dense_bytes"] = 4 * sum(b.length for b in tr.flat.buckets)
    out.update(_state(tr))
    if stop_at < STEPS:
        tr.save_checkpoint()
    tr.close()
    text = open(os.path.join(ckpt_dir, f"m{int(resume)}.rank{rank}.jsonl")).read()
    recs = [json.loads(line) for line in text.splitlines() if line.strip()]
    out["records"] = [r for r in recs if "payload_bytes_per_rank" in r]
    return out


@pytest.mark.parametrize("world", [2, 3])
def test_replicas_stages_and_log_records(tmp_path, world):
    res = run_world(_train, world, tmp_path, args=(str(tmp_path / "ck"), STEPS, False))
    r0 = res[0]
    assert r0["buckets"] > 1
    for r in res:
        assert r["start"] == 0 and r["kinds"] == ["none"] * TW + ["sign"] * (STEPS - TW)
        for name in ("params",) + STATE:
            assert torch.equal(r[name].view(torch.int32), r0[name].view(torch.int32)), name
        assert torch.equal(r["exp_avg_sq"].view(torch.int32), r["v_at_tw"].view(torch.int32))
        assert not torch.equal(r["exp_avg_sq_fresh"], r["exp_avg_sq"])
        assert float(r["resid"].abs().max()) > 0
        assert 0 < r["layout_bytes"] < r["dense_bytes"] // 20
        recs = {rec["step"]: rec for rec in r["records"]}
        assert sorted(recs) == list(range(1, STEPS + 1))
        for t, rec in recs.items():
            want = r["dense_bytes"] if t <= TW else r["layout_bytes"]
            assert rec["payload_bytes_per_rank"] == want, (t, rec["payload_bytes_per_rank"])
            assert 0 < rec["trust_ratio_min"] <= rec["trust_ratio_max"], t
    for r in res[1:]:
        assert not torch.equal(r["resid"], r0["resid"])  # per-rank state


def test_resume_in_the_compressed_stage(tmp_path):
    world = 2
    full = run_world(_train, world, tmp_path / "a", args=(str(tmp_path / "a" / "ck"), STEPS, False))
    ck = str(tmp_path / "b" / "ck")
    first = run_world(_train, world, tmp_path / "b1", args=(ck, 5, False))
    rest = run_world(_train, world, tmp_path / "b2", args=(ck, STEPS, True))
    for r, f, a in zip(rest, full, first):
        assert r["start"] == 5 and float(a["resid"].abs().max()) > 0
        assert r["kinds"] == ["sign", "sign"]
        for name in ("params", "resid") + STATE:
            assert torch.equal(r[name].view(torch.int32), f[name].view(torch.int32)), name
