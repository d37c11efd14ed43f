"""1-bit LAMB end to end on the GPU: LeNet on the golden MNIST images in full HIP-graph steps
(dense LAMB warm-up, then the sign-compressed momentum exchange with frozen trust ratios) against
the project's 96.5 % held-out floor (tests/e2e/test_gpu_accuracy.py); captured steps against eager
ones across the stage switch; and two Gloo ranks sharing ``cuda:0``.

The accuracies measured on one MI355X are in profiles/validation/onebit_lamb.md."""
import pytest
import torch

import ewdml
from ewdml import ops
from tests.distributed.helpers import run_world
from tests.golden_data import mnist_root

pytestmark = pytest.mark.gpu

FLOOR = 96.5  # the report's Method 5 LeNet figure (tests/e2e/test_gpu_accuracy.py)
STEPS, TW = 1500, 300
LENET = ["--network", "LeNet", "--dataset", "MNIST", "--data-dir", mnist_root(),
         "--holdout-from-test", "1000", "--batch-size", "64", "--lr", "0.003",
         "--eval-freq", "0", "--quiet", "--device", "cuda", "--hip-graph", "full",
         "--graph-warmup", "2", "--test-batch-size", "1000"]


def _run(flags, steps):
    from ewdml.runtime import Trainer

    torch.manual_seed(0)
    tr = Trainer(ewdml.parse_args(flags + ["--max-steps", str(steps)]))
    losses = []
    for _ in range(steps):
        loss, _ = tr.train_step()
        losses.append(loss)
    torch.cuda.synchronize()
    return tr, [float(v.detach()) for v in losses]


def test_lenet_real_mnist_onebit_lamb():
    ops.require()
    # the recipe first: dense LAMB at the same lr must clear the floor by a point, so that the
    # floor tests the compression and the frozen ratios and not the learning rate
    dense, _ = _run(LENET + ["--compress", "none", "--optimizer", "lamb"], STEPS)
    ev_dense = dense.evaluate()
    print(f"dense LAMB: holdout top-1 {ev_dense['top1']:.2f} %")
    assert ev_dense["top1"] >= FLOOR + 1.0, f"dense LAMB {ev_dense['top1']:.1f}%: fix the recipe"
    dense.close()
    tr, losses = _run(LENET + ["--compress", "sign", "--optimizer", "onebit_lamb",
                               "--onebit-warmup-steps", str(TW)], STEPS)
    assert tr.graph_mode == "full" and tr._graphs is not None
    assert tr.captures == 2  # the dense stage's graph, then the compressed stage's
    assert tr.exchange.codec.kind == "sign" and tr.opt.frozen and tr.opt.steps == STEPS
    assert int(tr.opt.step_t.item()) == STEPS
    assert all(v == v and abs(v) != float("inf") for v in losses)
    lo, hi = tr.opt.trust_ratio_range()
    f = tr.opt.last_factor
    print(f"trust ratios [{lo:.4f}, {hi:.4f}], factors [{float(f.min()):.3f}, "
          f"{float(f.max()):.3f}]")
    assert 0 < lo <= hi and 0.5 <= float(f.min()) and float(f.max()) <= 4.0
    ev = tr.evaluate()
    assert ev["samples"] == 1000
    print(f"1-bit LAMB (T_w = {TW}): holdout top-1 {ev['top1']:.2f} %")
    assert ev["top1"] >= FLOOR, f"holdout top-1 {ev['top1']:.1f}% < {FLOOR}%"


SYN = ["--network", "LeNet", "--dataset", "MNIST", "--batch-size", "32", "--synthetic-size",
       "1024", "--lr", "0.002", "--eval-freq", "0", "--quiet", "--device", "cuda", "--amp",
       "none", "--graph-warmup", "2", "--compress", "sign", "--optimizer", "onebit_lamb",
       "--weight-decay", "0.0005"]


def test_graph_matches_eager_across_the_switch():
    """T_w = 3, 8 steps: the warm-up's last step is a captured one, so the freeze it leaves (the
    fresh variance, r_frozen) comes out of a replay; the compressed stage is re-captured once."""
    ops.require()
    flags = SYN + ["--onebit-warmup-steps", "3"]
    ref, _ = _run(flags + ["--hip-graph", "off"], 8)
    tr, _ = _run(flags + ["--hip-graph", "full"], 8)
    assert tr.graph_mode == "full" and tr._graphs is not None and tr.captures == 2
    assert ref.exchange.codec.kind == tr.exchange.codec.kind == "sign"
    assert torch.equal(tr.opt.step_t, ref.opt.step_t) and int(tr.opt.step_t.item()) == 8
    rel = float((tr.flat.data - ref.flat.data).norm() / ref.flat.data.norm())
    print(f"graph vs eager over the switch: rel {rel:.3e}")
    for name in ("r_frozen", "coeff_ema", "exp_avg_sq", "exp_avg_sq_fresh", "exp_avg", "ratio",
                 "_factors"):
        a, b = getattr(tr.opt, name), getattr(ref.opt, name)
        assert torch.equal(a.view(torch.int32), b.view(torch.int32)), name
    assert torch.equal(tr.flat.data.view(torch.int32), ref.flat.data.view(torch.int32))
    assert not torch.equal(tr.opt.exp_avg_sq_fresh, tr.opt.exp_avg_sq)


def _train(rank, world, steps):
    import os

    os.environ["LOCAL_RANK"] = "0"  # both ranks share the box's one GPU
    from ewdml.parallel.engine import replica_fingerprint
    from ewdml.runtime import Trainer

    torch.cuda.set_device(0)
    ops.require()
    flags = [f for f in SYN if f not in ("--graph-warmup", "2")]
    tr = Trainer(ewdml.parse_args(flags + ["--graph-warmup", "1", "--onebit-warmup-steps", "2",
                                           "--batch-size", "16", "--max-steps", str(steps)]))
    before = tr.flat.data.clone()
    kinds, losses = [], []
    for _ in range(steps):
        loss, _ = tr.train_step()
        losses.append(float(loss.detach()))
        kinds.append(tr.exchange.codec.kind)
    torch.cuda.synchronize()
    return {"fp": replica_fingerprint(tr.flat.data), "m": replica_fingerprint(tr.opt.exp_avg),
            "vf": replica_fingerprint(tr.opt.exp_avg_sq_fresh),
            "ratio": tr.opt.ratio.cpu(), "factors": tr.opt._factors.cpu(),
            "losses": losses, "kinds": kinds, "moved": not torch.equal(before, tr.flat.data),
            "bytes": tr.exchange.last.payload_bytes,
            "resid": replica_fingerprint(tr.exchange.resid)}


def test_two_ranks_on_one_gpu_identical(tmp_path):
    res = run_world(_train, 2, tmp_path, args=(6,))

    def key(fp):
        return (repr(fp["sum"]), repr(fp["wsum"]), fp["xor"])

    for name in ("fp", "m", "vf"):
        assert key(res[0][name]) == key(res[1][name]), name
    assert torch.equal(res[0]["ratio"], res[1]["ratio"])
    assert torch.equal(res[0]["factors"], res[1]["factors"])
    assert key(res[0]["resid"]) != key(res[1]["resid"])
    for r in res:
        assert r["kinds"] == ["none"] * 2 + ["sign"] * 4
        assert r["moved"] and all(l == l for l in r["losses"])
        assert r["bytes"] == res[0]["bytes"] > 0
