"""The Hadamard-rotated sign codec end to end on the GPU (``--compress sign --sign-rotate
hadamard``): three trainer steps of LeNet whose every encode and fused decode + SGD step is bitwise
the CPU oracle's on the trainer's own gradients, one captured graph under ``--hip-graph auto``, and
LeNet on the golden MNIST images against the project's 96.5 % held-out floor with the settings of
the unrotated codec's test (tests/e2e/test_sign_train_gpu.py)."""
import pytest
import torch

import ewdml
from ewdml import ops
from ewdml.compress import oracle
from tests.golden_data import mnist_root

pytestmark = pytest.mark.gpu

ROT = ["--compress", "sign", "--sign-rotate", "hadamard"]
# lr = 2^-4 and dampening = 0: the oracle's SGD step does not depend on whether torch's CPU
# add_(alpha=) contracts its multiply-add (tests/kernels/test_sign_rotate_hip.py)
SYN = ["--network", "LeNet", "--dataset", "MNIST", "--batch-size", "32", "--synthetic-size",
       "1024", "--lr", "0.0625", "--momentum", "0.9", "--eval-freq", "0", "--quiet", "--device",
       "cuda", "--amp", "none", "--graph-warmup", "2"] + ROT


def _trainer(flags, steps):
    from ewdml.runtime import Trainer

    torch.manual_seed(0)
    return Trainer(ewdml.parse_args(flags + ["--max-steps", str(steps)]))


def _bits_equal(a, b):
    return torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def test_three_steps_bitwise_the_oracle_path():
    """Every encode and every decode + step of three eager trainer steps is replayed on the CPU
    through the oracle from the same gradients: payloads, residuals, parameters and momenta are
    bitwise equal, so the trainer's parameters are the oracle path's."""
    ops.require()
    tr = _trainer(SYN + ["--hip-graph", "off"], 3)
    ex, codec = tr.exchange, tr.exchange.codec
    assert codec.describe() == "sign1b-h" and ex.ef_mode == "plain" and ex.resid is not None
    shadow = {"p": tr.flat.data.cpu().clone(), "m": torch.zeros(tr.flat.numel),
              "r": torch.zeros(tr.flat.numel), "calls": 0}
    real_encode, real_apply = codec.encode, codec.decode_apply_sgd
    buckets = {b.index: b for b in tr.flat.buckets}

    def encode(b, grad, payload, step, rank, resid=None, **kw):
        plan, lay, bk = codec.plans[b], codec.layouts[b], buckets[b]
        if isinstance(grad, (list, tuple)):
            g = torch.zeros(plan.length)
            for t, off, n in zip(grad, plan.offsets, plan.numels):
                t = t.detach()
                if t.dim() == 4 and not t.is_contiguous():  # channels_last: memory order
                    t = t.permute(0, 2, 3, 1)
                g[off:off + n] = t.float().reshape(-1).cpu()
        else:
            g = grad.detach().float().cpu().clone()
        r = shadow["r"][bk.start:bk.start + bk.length]
        assert _bits_equal(resid.cpu(), r), "residual before the encode"
        real_encode(b, grad, payload, step, rank, resid=resid, **kw)
        ref = oracle.encode_sign(g, plan, lay, r, codec.rot_key(b))
        assert torch.equal(payload[:lay.nbytes].cpu(), ref), f"bucket {b}: payload"
        assert _bits_equal(resid.cpu(), r), f"bucket {b}: residual"
        shadow["calls"] += 1

    def apply(b, recv, scale, param, mom, hp, first, **kw):
        plan, lay, bk = codec.plans[b], codec.layouts[b], buckets[b]
        sl = slice(bk.start, bk.start + bk.length)
        g = oracle.decode_sum(recv.cpu(), plan, lay, 0, scale, codec.rot_key(b))
        real_apply(b, recv, scale, param, mom, hp, first, **kw)
        p, m = shadow["p"][sl], shadow["m"][sl]
        for off, n in zip(plan.offsets, plan.numels):
            oracle.sgd_apply(p[off:off + n], m[off:off + n], g[off:off + n], hp["lr"],
                             hp["momentum"], hp["dampening"], hp["weight_decay"], hp["nesterov"],
                             first)
        for off, n in zip(plan.offsets, plan.numels):
            assert _bits_equal(param[off:off + n].cpu(), p[off:off + n]), f"bucket {b}: params"
            assert _bits_equal(mom[off:off + n].cpu(), m[off:off + n]), f"bucket {b}: momentum"

    codec.encode, codec.decode_apply_sgd = encode, apply
    before = tr.flat.data.clone()
    for _ in range(3):
        loss, _ = tr.train_step()
        assert torch.isfinite(loss.detach()).item()
    torch.cuda.synchronize()
    assert shadow["calls"] == 3 * len(tr.flat.buckets)
    assert not torch.equal(before, tr.flat.data) and float(ex.resid.abs().max()) > 0
    tr.close()


def test_one_capture_and_graph_matches_eager():
    ops.require()
    ref = _trainer(SYN + ["--hip-graph", "off"], 10)
    tr = _trainer(SYN + ["--hip-graph", "auto"], 10)
    for t in (ref, tr):
        for _ in range(10):
            t.train_step()
    torch.cuda.synchronize()
    assert tr.graph_mode == "full" and tr._graphs is not None and tr.captures == 1
    # LeNet's MIOpen convolutions are not bitwise between eager and captured runs: the bound of
    # tests/e2e/test_lion_gpu.py test_graph_matches_eager
    rel = float((tr.flat.data - ref.flat.data).norm() / ref.flat.data.norm())
    print(f"graph vs eager: rel {rel:.3e}")
    assert rel < 1e-3, f"params differ from eager by {rel:.2e}"
    ref.close()
    tr.close()


LENET = ["--network", "LeNet", "--dataset", "MNIST", "--data-dir", mnist_root(),
         "--holdout-from-test", "1000", "--batch-size", "64", "--lr", "0.01", "--momentum", "0.9",
         "--eval-freq", "0", "--quiet", "--device", "cuda", "--hip-graph", "full",
         "--graph-warmup", "2", "--test-batch-size", "1000"]


def test_lenet_real_mnist_rotated_sign():
    ops.require()
    steps = 1500
    tr = _trainer(LENET + ROT, steps)
    assert tr.exchange.ef_mode == "plain" and tr.exchange.codec.rotate == "hadamard"
    losses = []
    for _ in range(steps):
        loss, _ = tr.train_step()
        losses.append(loss)
    torch.cuda.synchronize()
    assert tr.graph_mode == "full" and tr._graphs is not None and tr.captures == 1
    assert all(torch.isfinite(v.detach()).item() for v in losses)
    ev = tr.evaluate()
    assert ev["samples"] == 1000
    print(f"rotated sign codec: holdout top-1 {ev['top1']:.2f} %")
    tr.close()
    assert ev["top1"] >= 96.5, f"holdout top-1 {ev['top1']:.1f}% < 96.5%"
