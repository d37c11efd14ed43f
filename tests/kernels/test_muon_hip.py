"""Muon's kernels (ops/csrc/muon.hip) through ``FlatMuon.step_range`` on the GPU, against
``compress/oracle.py muon_apply`` in float64.  One step over a flat buffer of one matrix and a
bias; with D the matrix's update (new - old), ``|D_hip - D_64| <= 3 |D_oracle - D_64|``: the
oracle's own error in the same precision is the yardstick (floor ``2^-23 |D_64|`` where it is 0).
The momentum and the bias are bitwise the oracle's."""
import functools

import pytest
import torch

import ewdml
from ewdml import ops
from ewdml.compress import oracle
from ewdml.optim import FlatMuon
from tests.layerwise_ref import make_flat, make_grad

pytestmark = pytest.mark.gpu

KW = dict(lr=0.02, momentum=0.9, weight_decay=1e-2, nesterov=True, aux_lr=0.005)
# below one MFMA tile | c below one k-step, both ragged | two row tiles: mirrored gram tiles |
# the gram's slab split, ragged r | tall: strided | square | zero gradient and momentum
SHAPES = [(10, 500), (20, 25), (80, 1152), (48, 4608), (800, 50), (256, 256), "zero"]


def _start(shape, device):
    zero = shape == "zero"
    shape = (20, 25) if zero else shape
    flat = make_flat(shapes=[shape, (shape[0],)], seed=3, device=device)
    grad, mom = make_grad(flat, 0), make_grad(flat, 7)
    if zero:
        grad[:shape[0] * shape[1]] = 0
        mom[:shape[0] * shape[1]] = 0
    return flat, grad, mom, shape[0] * shape[1]


@functools.lru_cache(maxsize=None)
def _cpu(shape, ns_dtype, ns_steps):
    """(start, fp32 oracle's, float64's) parameters and the oracle's momentum."""
    flat, grad, mom, _ = _start(shape, "cpu")
    p0 = flat.data.clone()
    opt = FlatMuon(flat, ns_steps=ns_steps, ns_dtype=ns_dtype, **KW)
    opt.mom.copy_(mom)
    p64, m64 = p0.double(), mom.double()
    oracle.muon_apply(p64, m64, grad.double() * 0.5, [(o, p.numel(), r) for o, p, r in zip(
        flat.offsets, flat.params, opt.rows)], KW["lr"], KW["momentum"], KW["weight_decay"],
        KW["nesterov"], opt.aux_ratio, ns_steps, "fp32")
    opt.step(grad=grad, grad_scale=0.5)
    return p0, flat.data, p64, opt.mom


def _hip(shape, ns_dtype, ns_steps, graph=False):
    ops.require()
    flat, grad, mom, _ = _start(shape, "cuda")
    opt = FlatMuon(flat, ns_steps=ns_steps, ns_dtype=ns_dtype, **KW)
    opt.mom.copy_(mom)
    if graph:
        p0 = flat.data.clone()
        opt.step_range(0, flat.numel, grad, 0.5)  # warm up, then back to the start
        flat.data.copy_(p0)
        opt.mom.copy_(mom)
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, capture_error_mode="thread_local"):
            opt.step_range(0, flat.numel, grad, 0.5)
        g.replay()
    else:
        opt.step_range(0, flat.numel, grad, 0.5)
    torch.cuda.synchronize()
    assert bool(torch.isfinite(flat.data).all())
    return flat.data.cpu(), opt.mom.cpu()


def _check(shape, ns_dtype, ns_steps):
    p0, p32, p64, m32 = _cpu(shape, ns_dtype, ns_steps)
    p, m = _hip(shape, ns_dtype, ns_steps)
    n = _start(shape, "cpu")[3]
    d64 = p64[:n] - p0[:n].double()
    err = float((p[:n].double() - p0[:n].double() - d64).norm())
    ref = float((p32[:n].double() - p0[:n].double() - d64).norm())
    bound = 3 * ref if ref > 0 else 2.0 ** -23 * float(d64.norm())
    print(f"muon {shape} {ns_dtype} steps={ns_steps}: hip {err:.3e} oracle {ref:.3e} "
          f"ratio {err / ref if ref > 0 else float('nan'):.3f} |D| {float(d64.norm()):.3e}")
    assert err <= bound
    assert torch.equal(m.view(torch.int32), m32.view(torch.int32)), "momentum"
    assert torch.equal(p[n:].view(torch.int32), p32[n:].view(torch.int32)), "bias"


@pytest.mark.parametrize("ns_dtype", ["fp32", "bf16"])
@pytest.mark.parametrize("shape", SHAPES, ids=str)
def test_one_step_within_three_oracle_errors(shape, ns_dtype):
    _check(shape, ns_dtype, 5)


@pytest.mark.parametrize("ns_steps", [1, 3])
def test_other_step_counts(ns_steps):
    """The X ping-pong's parity and the last iteration's epilogue."""
    _check((80, 1152), "fp32", ns_steps)


def test_two_runs_are_bitwise_equal():
    """The gram's slabs are summed in slab order by whichever block arrives last."""
    a, b = _hip((48, 4608), "fp32", 5), _hip((48, 4608), "fp32", 5)
    assert torch.equal(a[0].view(torch.int32), b[0].view(torch.int32))


def test_captured_replay_equals_the_eager_step():
    a, b = _hip((48, 4608), "bf16", 5), _hip((48, 4608), "bf16", 5, graph=True)
    assert torch.equal(a[0].view(torch.int32), b[0].view(torch.int32))
    assert torch.equal(a[1].view(torch.int32), b[1].view(torch.int32))


def test_lenet_trains_and_resumes_bitwise(tmp_path):
    from ewdml.runtime import Trainer

    flags = ["--network", "LeNet", "--dataset", "MNIST", "--batch-size", "16", "--synthetic-size",
             "1024", "--eval-freq", "0", "--quiet", "--device", "cuda", "--amp", "none",
             "--optimizer", "muon", "--lr", "0.02", "--momentum", "0.9", "--nesterov",
             "--hip-graph", "off", "--no-legacy-ckpt", "--max-steps", "20"]

    def trainer(extra):
        torch.manual_seed(0)
        return Trainer(ewdml.parse_args(flags + extra))

    full = trainer(["--train-dir", str(tmp_path / "a")])
    losses = [float(full.train_step()[0].detach()) for _ in range(20)]
    assert all(l == l and abs(l) != float("inf") for l in losses) and losses[-1] < losses[0]
    first = trainer(["--train-dir", str(tmp_path / "b")])
    for _ in range(10):
        first.train_step()
    first.save_checkpoint()
    rest = trainer(["--train-dir", str(tmp_path / "b"), "--resume"])
    assert rest.step == 10
    while rest.step < 20:
        rest.train_step()
    torch.cuda.synchronize()
    assert torch.equal(rest.flat.data.view(torch.int32), full.flat.data.view(torch.int32))
