"""The count-sketch exchange end to end on the GPU (``--compress sketch``): LeNet on the synthetic
MNIST-shaped set at batch 64, 20 steps with ``--hip-graph auto`` (split graphs) against the same
run through the torch oracle (``compress/oracle.py sketch_*``, the CPU execution path, here run
eagerly on the same device so that forward and backward are the same kernels), bit for bit in
parameters, momentum and residual; one capture of two graphs; a falling loss; the log record's
payload bytes against the byte formula."""
import pytest
import torch

import ewdml
from ewdml import ops
from ewdml.compress import codecs
from ewdml.utils.metrics import byte_summary
from tests.sketch_sim import same_bits

pytestmark = pytest.mark.gpu

STEPS = 20
# lr and momentum are powers of two: the oracle's torch step and the kernel's agree bit for bit
# whether or not a multiply-add is fused
SYN = ["--network", "LeNet", "--dataset", "MNIST", "--batch-size", "64", "--synthetic-size",
       "2048", "--eval-freq", "0", "--quiet", "--device", "cuda", "--amp", "none", "--lr", "0.0625",
       "--momentum", "0.5", "--graph-warmup", "2", "--compress", "sketch", "--no-legacy-ckpt",
       "--max-steps", str(STEPS)]


def _run(flags):
    from ewdml.runtime import Trainer

    torch.manual_seed(0)
    tr = Trainer(ewdml.parse_args(flags))
    losses = []
    while tr.step < STEPS:
        loss, _ = tr.train_step()
        losses.append(loss.detach().clone())
    torch.cuda.synchronize()
    return tr, [float(v) for v in losses]


def test_split_graph_steps_equal_the_oracle_path_bitwise(monkeypatch):
    from ewdml.parallel.sketch import SketchExchange

    ops.require()
    tr, losses = _run(SYN + ["--hip-graph", "auto"])
    assert isinstance(tr.exchange, SketchExchange) and tr.flat.attach_grads
    assert tr.exchange.codec.sk_dev is not None  # the kernels ran, not the oracle
    assert tr.graph_mode == "split" and tr._graphs is not None and len(tr._graphs) == 2
    assert tr.captures == 1
    monkeypatch.setattr(codecs, "_FORCE_ORACLE", True)
    ref, ref_losses = _run(SYN + ["--hip-graph", "off"])
    assert ref.graph_mode == "off" and ref.exchange.codec.sk_dev is None
    assert same_bits(tr.flat.data, ref.flat.data), "parameters"
    assert same_bits(tr.opt.mom, ref.opt.mom), "momentum"
    assert same_bits(tr.exchange.resid, ref.exchange.resid), "residual"
    assert float(tr.exchange.resid.abs().max()) > 0
    assert losses == ref_losses and all(v == v for v in losses)
    print(f"loss {losses[0]:.4f} -> {losses[-1]:.4f}")
    assert losses[-1] < losses[0]
    # payload = 4 (R W + K + dense elements) per bucket: LeNet's 431,080 parameters at 1 %
    sk = tr.exchange.sk
    assert tr.exchange.codec.describe() == "sketch-r3"
    want = sum(4 * (3 * t.W + t.K + t.dense_elems) for t in sk)
    rec = byte_summary(tr.exchange.last, tr.world)
    assert rec["payload_bytes_per_rank"] == want
    assert rec["wire_bytes_sent_per_rank"] == 0  # a world of one: 2 (N - 1) / N = 0
    assert all(t.W == 8192 * -(-2 * t.K // 8192) for t in sk)
