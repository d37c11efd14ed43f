"""APOLLO on the CPU: the fp32 oracle (``compress/oracle.py apollo_apply``) against itself in
float64 across a projection epoch, ``FlatApollo``'s state and the command line."""
import pytest
import torch

import ewdml
from ewdml.compress import oracle
from ewdml.optim import FlatApollo, FlatGalore, make_optimizer
from tests.layerwise_ref import make_flat, make_grad

BASE = ["--network", "LeNet", "--dataset", "MNIST", "--batch-size", "16", "--synthetic-size",
        "256", "--eval-freq", "0", "--quiet", "--device", "cpu", "--log-interval", "1000"]


@pytest.mark.parametrize("rank,scale_type", [(16, "channel"), (16, "tensor"), (1, "tensor")])
def test_fp32_oracle_follows_float64_across_an_epoch(rank, scale_type):
    hp = dict(lr=0.01, rank=rank, update_gap=2, scale_type=scale_type, weight_decay=0.01, seed=3)
    flat = make_flat(shapes=[(20, 31), (31, 20), (16, 9), (37,)], seed=5)
    opt = FlatApollo(flat, **hp)
    tensors = opt._tensors(0, flat.numel)
    assert [bool(n) for _, _, n, *_ in tensors] == [True, True, rank == 1, False]
    p64, st64 = flat.data.double(), [x.double() for x in opt._state(0, 4)]
    for t in (1, 2, 3):  # the signs change at step 3; the limiter has a previous norm from step 2
        g = make_grad(flat, t)
        oracle.apollo_apply(p64, *st64, g.double() * 0.5, tensors, step=t, **hp)
        opt.step(grad=g, grad_scale=0.5)
    assert bool((st64[4] > 0).all()) and bool(torch.isfinite(p64).all())
    # fp32 sums of at most 31 terms, and s_j a ratio of such sums: 1e-4 (about 800 ulp) leaves
    # room for the cancellation in R = sum of +-g, where a wrong sign bit, epoch or limiter moves
    # the step lr s_j g itself, 1e-2 of p or more
    torch.testing.assert_close(flat.data.double(), p64, rtol=1e-4, atol=1e-6)
    for got, want in zip(opt._state(0, 4), st64):
        torch.testing.assert_close(got.double(), want, rtol=1e-4, atol=1e-7)
    # P has exact +-1 signs that differ between epochs and tensors
    S = [oracle.apollo_signs(3, gi, e, 20, 16) for gi, e in ((0, 0), (0, 1), (1, 0))]
    assert all(bool((s.abs() == 1).all()) for s in S)
    assert not torch.equal(S[0], S[1]) and not torch.equal(S[0], S[2])


def test_state_is_below_galores_and_resumes_bitwise():
    flats = [make_flat(bucket_bytes=4 * 8192) for _ in range(4)]
    full, first, rest = (make_optimizer("apollo", f, lr=0.01, apollo_rank=16, apollo_update_gap=3,
                                        weight_decay=0.01, seed=7) for f in flats[:3])
    assert isinstance(full, FlatApollo) and not full.fusable and len(flats[0].buckets) >= 2
    assert full.kind == "apollo" and full.seed == 7 and not hasattr(full, "proj")
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
    assert sd["kind"] == "apollo" and sd["steps"] == 2 and "proj" not in sd
    flats[2].data.copy_(flats[1].data)
    rest.seed = 0  # the checkpoint's seed wins
    rest.load_state_dict(sd)
    for s in range(2, 5):
        rest.step(grad=make_grad(flats[2], s))
    assert torch.equal(flats[2].data.view(torch.int32), flats[0].data.view(torch.int32))
    for k in FlatApollo._STATE:
        assert torch.equal(getattr(rest, k), getattr(full, k)), k
    # layerwise_ref.SHAPES at rank 16: only (64, 128) is projected, 2 r l floats and two norms;
    # the rest keeps two full moments, each tensor padded to 4 floats
    dense = 12 + 24 + 8196 + 20000
    assert full.state_bytes() == 4 * (2 * 16 * 128 + 2 + 2 * dense)
    assert full.state_bytes() < FlatGalore(flats[3], rank=16).state_bytes()


@pytest.mark.parametrize("flags,match", [
    (["--apollo-rank", "32"], "belongs to --optimizer apollo"),
    (["--optimizer", "adam", "--apollo-update-gap", "5"], "belongs to --optimizer apollo"),
    (["--optimizer", "galore", "--apollo-scale", "0.5"], "belongs to --optimizer apollo"),
    (["--optimizer", "adam", "--apollo-scale-type", "tensor"], "belongs to --optimizer apollo"),
    (["--optimizer", "apollo", "--apollo-rank", "24"], "--apollo-rank must be 1 or a multiple"),
    (["--optimizer", "apollo", "--apollo-rank", "144"], "--apollo-rank must be 1 or a multiple"),
    (["--optimizer", "apollo", "--apollo-update-gap", "0"], "--apollo-update-gap must be >= 1"),
    (["--optimizer", "apollo", "--apollo-scale", "0"], "--apollo-scale must be > 0")])
def test_cli_refusals(flags, match):
    with pytest.raises(ValueError, match=match):
        ewdml.parse_args(BASE + flags)


def test_cli_resolves():
    c = ewdml.parse_args(BASE + ["--optimizer", "apollo"])
    assert (c.apollo_rank, c.apollo_update_gap, c.apollo_scale, c.apollo_scale_type) == (
        64, 200, 1.0, "channel")
    c = ewdml.parse_args(BASE + ["--optimizer", "apollo", "--apollo-rank", "1",
                                 "--apollo-scale-type", "tensor", "--apollo-scale", "128"])
    assert (c.apollo_rank, c.apollo_scale, c.apollo_scale_type) == (1, 128.0, "tensor")
