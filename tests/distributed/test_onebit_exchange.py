"""1-bit Adam through the trainer on CPU/Gloo: 2 and 3 ranks train LeNet for T_w = 3 dense Adam
steps and 4 compressed-stage steps; replicas and the shared momentum stay bitwise identical, the
variance is frozen, the payload drops to the sign layouts, and a checkpoint taken inside the
compressed stage resumes bit for bit."""
import pytest
import torch

from .helpers import run_world

pytestmark = pytest.mark.slow

TW, STEPS = 3, 7
BASE = ["--network", "LeNet", "--dataset", "MNIST", "--batch-size", "16", "--synthetic-size",
        "512", "--lr", "0.001", "--eval-freq", "0", "--quiet", "--device", "cpu",
        "--log-interval", "1000", "--compress", "sign", "--optimizer", "onebit_adam",
        "--onebit-warmup-steps", str(TW), "--no-legacy-ckpt"]


def _state(tr):
    return {"params": tr.flat.data.clone(), "exp_avg": tr.opt.exp_avg.clone(),
            "exp_avg_sq": tr.opt.exp_avg_sq.clone(), "resid": tr.exchange.resid.clone()}


def _train(rank, world, ckpt_dir, stop_at, resume):
    """Steps up to ``stop_at`` (checkpoint there), or -- ``resume`` -- from the checkpoint on."""
    import ewdml
    from ewdml.runtime import Trainer

    args = BASE + ["--max-steps", str(STEPS), "--train-dir", ckpt_dir]
    tr = Trainer(ewdml.parse_args(args + (["--resume"] if resume else [])))
    out = {"start": tr.step, "stats": [], "v_at_tw": None}
    while tr.step < stop_at:
        tr.train_step()
        st = tr.exchange.last
        out["stats"].append((tr.exchange.codec.kind, st.payload_bytes, st.wire_bytes_recv))
        if tr.step == TW:
            out["v_at_tw"] = tr.opt.exp_avg_sq.clone()
    out["layout_bytes"] = sum(lay.nbytes for lay in tr.exchange.codec.layouts)
    out["dense_bytes"] = 4 * sum(b.length for b in tr.flat.buckets)
    out.update(_state(tr))
    if stop_at < STEPS:
        tr.save_checkpoint()
    tr.close()
    return out


@pytest.mark.parametrize("world", [2, 3])
def test_onebit_replicas_and_stages(tmp_path, world):
    res = run_world(_train, world, tmp_path, args=(str(tmp_path / "ck"), STEPS, False))
    r0 = res[0]
    for r in res:
        assert r["start"] == 0 and len(r["stats"]) == STEPS
        for name in ("params", "exp_avg", "exp_avg_sq"):
            assert torch.equal(r[name].view(torch.int32), r0[name].view(torch.int32)), name
        assert torch.equal(r["exp_avg_sq"].view(torch.int32), r["v_at_tw"].view(torch.int32))
        assert float(r["resid"].abs().max()) > 0
        for t, (kind, payload, recv) in enumerate(r["stats"], 1):
            if t <= TW:
                assert kind == "none" and payload == r["dense_bytes"]
            else:
                assert kind == "sign" and payload == r["layout_bytes"]
                assert recv == (world - 1) * r["layout_bytes"]
        assert 0 < r["layout_bytes"] < r["dense_bytes"] // 20
    for r in res[1:]:
        assert not torch.equal(r["resid"], r0["resid"])  # per-rank state


def test_onebit_resume_in_the_compressed_stage(tmp_path):
    world = 2
    full = run_world(_train, world, tmp_path / "a", args=(str(tmp_path / "a" / "ck"), STEPS, False))
    ck = str(tmp_path / "b" / "ck")
    first = run_world(_train, world, tmp_path / "b1", args=(ck, 5, False))
    rest = run_world(_train, world, tmp_path / "b2", args=(ck, STEPS, True))
    for r, f, a in zip(rest, full, first):
        assert r["start"] == 5 and float(a["resid"].abs().max()) > 0
        assert [s[0] for s in r["stats"]] == ["sign", "sign"]
        for name in ("params", "exp_avg", "exp_avg_sq", "resid"):
            assert torch.equal(r[name].view(torch.int32), f[name].view(torch.int32)), name
