"""GaLore on the CPU: the torch oracle (``compress/oracle.py galore_apply``) in double against the
rule written out per tensor with explicit loops, ``FlatGalore``'s state and the command line."""
import pytest
import torch

import ewdml
from ewdml.compress import oracle
from ewdml.optim import FlatGalore, make_optimizer
from tests.layerwise_ref import make_flat, make_grad

BASE = ["--network", "LeNet", "--dataset", "MNIST", "--batch-size", "16", "--synthetic-size",
        "256", "--eval-freq", "0", "--quiet", "--device", "cpu", "--log-interval", "1000"]
HP = dict(lr=0.01, rank=16, update_gap=2, scale=0.25, weight_decay=0.01)


def _orth(Y):
    """Gram-Schmidt twice per column, one dot at a time."""
    Q = torch.zeros_like(Y)
    for c in range(Y.shape[1]):
        y, before = Y[:, c].clone(), float(Y[:, c].norm())
        for sweep in range(2):
            y = y - sum(Q[:, j] * float(Q[:, j] @ y) for j in range(c))
            if sweep == 0 and float(y.norm()) <= before / 4096:
                break
        else:
            Q[:, c] = y / y.norm()
    return Q


def _plain(W, st, G, t, lr, rank, update_gap, scale, weight_decay):
    """The issue's rule for one tensor in float64, in the tensor's own orientation."""
    b1, b2, eps = 0.9, 0.999, 1e-8
    n, m = W.shape if W.dim() == 2 else (1, 1)
    if min(n, m) > rank:
        if (t - 1) % update_gap == 0:
            for _ in range(2):
                Z = G.t() @ st["P"] if n <= m else G @ st["P"]
                st["P"] = _orth(G @ Z if n <= m else G.t() @ Z)
        R = st["P"].t() @ G if n <= m else G @ st["P"]
    else:
        R, scale = G, 1.0
    st["M"] = b1 * st["M"] + (1 - b1) * R
    st["V"] = b2 * st["V"] + (1 - b2) * R * R
    N = (st["M"] / (1 - b1 ** t)) / ((st["V"] / (1 - b2 ** t)).sqrt() + eps)
    if min(n, m) > rank:
        N = st["P"] @ N if n <= m else N @ st["P"].t()
    return W * (1 - lr * weight_decay) - lr * scale * N


@pytest.mark.parametrize("shape", [(20, 31), (31, 20)])
def test_oracle_in_double_follows_the_rule(shape):
    flat = make_flat(shapes=[shape, (16, 9), (37,)], seed=5)
    opt = FlatGalore(flat, **HP)
    tensors = opt._tensors(0, flat.numel)
    assert [bool(n) for _, _, n, _, _ in tensors] == [True, False, False]
    s, l = min(shape), max(shape)
    ws = [p.detach().double() for p in flat.params]
    sts = [dict(P=opt.proj.double().view(s, 16), M=0.0, V=0.0), dict(M=0.0, V=0.0),
           dict(M=0.0, V=0.0)]
    p64, st64 = flat.data.double(), [x.double() for x in opt._state(0, 3)]
    for t in (1, 2, 3):  # refresh, keep, refresh from a warm start
        g = make_grad(flat, t).double() * 0.5
        oracle.galore_apply(p64, *st64, g, tensors, step=t, **HP)
        for i, (off, numel, *_) in enumerate(tensors):
            ws[i] = _plain(ws[i], sts[i], g[off:off + numel].view(ws[i].shape), t, **HP)
            torch.testing.assert_close(p64[off:off + numel], ws[i].reshape(-1), rtol=1e-6,
                                       atol=1e-8)
    # the fp32 path steps the same way to fp32 accuracy
    for t in (1, 2, 3):
        opt.step(grad=make_grad(flat, t), grad_scale=0.5)
    torch.testing.assert_close(flat.data.double(), p64, rtol=1e-4, atol=1e-6)


def test_state_is_low_rank_and_resumes_bitwise():
    flats = [make_flat(bucket_bytes=4 * 8192) for _ in range(3)]
    full, first, rest = (make_optimizer("galore", f, lr=0.01, galore_rank=16, galore_update_gap=3,
                                        weight_decay=0.01) for f in flats)
    assert isinstance(full, FlatGalore) and not full.fusable and len(flats[0].buckets) >= 2
    assert full.kind == "galore"
    with pytest.raises(ValueError, match="a bucket or the whole model"):
        full.step_range(0, 64, flats[0].grad[:64])
    for s in range(5):
        full.step(grad=make_grad(flats[0], s))
    for s in range(2):  # per bucket, as the exchanges step
        g = make_grad(flats[1], s)
        for b in flats[1].buckets:
            first.step_range(b.start, b.length, g[b.start:b.start + b.length])
        first.end_step()
    sd = {k: (v.clone() if torch.is_tensor(v) else v) for k, v in first.state_dict().items()}
    assert sd["kind"] == "galore" and sd["steps"] == 2
    flats[2].data.copy_(flats[1].data)
    rest.load_state_dict(sd)
    for s in range(2, 5):
        rest.step(grad=make_grad(flats[2], s))
    assert torch.equal(flats[2].data.view(torch.int32), flats[0].data.view(torch.int32))
    assert torch.equal(rest.proj, full.proj) and torch.equal(rest.m_lr, full.m_lr)
    # layerwise_ref.SHAPES at rank 16: only (64, 128) is projected, s r + 2 r l floats; the rest
    # keeps two full moments, each tensor padded to 4 floats
    dense = 12 + 24 + 8196 + 20000
    assert full.state_bytes() == 4 * (64 * 16 + 2 * 16 * 128 + 2 * dense)


@pytest.mark.parametrize("flags,match", [
    (["--galore-rank", "32"], "belongs to --optimizer galore"),
    (["--optimizer", "adam", "--galore-update-gap", "5"], "belongs to --optimizer galore"),
    (["--optimizer", "adam", "--galore-scale", "0.5"], "belongs to --optimizer galore"),
    (["--optimizer", "galore", "--galore-rank", "24"], "--galore-rank must be a multiple of 16"),
    (["--optimizer", "galore", "--galore-rank", "144"], "--galore-rank must be a multiple of 16"),
    (["--optimizer", "galore", "--galore-update-gap", "0"], "--galore-update-gap must be >= 1"),
    (["--optimizer", "galore", "--galore-scale", "0"], "--galore-scale must be > 0")])
def test_cli_refusals(flags, match):
    with pytest.raises(ValueError, match=match):
        ewdml.parse_args(BASE + flags)


def test_cli_resolves():
    c = ewdml.parse_args(BASE + ["--optimizer", "galore", "--galore-rank", "32"])
    assert (c.galore_rank, c.galore_update_gap, c.galore_scale) == (32, 200, 0.25)
