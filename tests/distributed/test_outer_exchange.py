"""``--outer-optimizer`` through the trainer on CPU / Gloo, worlds of 2 and 3: LeNet on synthetic
data, a sync every 3 steps, 9 steps.

Every rank spies on its own sync steps.  The delta that enters the outer step must be the mean of
the ranks' decoded deltas (under ``--select-best`` the winner's decoded delta): for a compressing
codec each rank decodes every row of the all-gather on its own and averages them in rank order,
bit for bit what the exchange delivers; for ``--compress none`` the ranks' own deltas are gathered
and their mean must agree within the roundings of a three-term fp32 sum taken in any order, which
is what Gloo's all-reduce leaves open.  From there a simulation that knows only the first anchor
and the deltas calls ``oracle.outer_apply`` and must reproduce anchor, weights and momentum of
every sync bit for bit.
"""
import pytest
import torch

from .helpers import run_world

pytestmark = pytest.mark.slow

EVERY, STEPS = 3, 9
BASE = ["--network", "LeNet", "--dataset", "MNIST", "--batch-size", "16", "--synthetic-size",
        "512", "--momentum", "0.9", "--lr", "0.05", "--quiet", "--device", "cpu",
        "--log-interval", "1000", "--eval-freq", "0", "--sync-every", str(EVERY), "--sync-mode",
        "model", "--max-steps", str(STEPS)]
DILOCO = ["--outer-optimizer", "nesterov", "--outer-lr", "0.7", "--outer-momentum", "0.9"]
U = 2.0 ** -24


def _bits(t):
    return t.contiguous().view(torch.int32)


def _run(flags, spy=False):
    """One trainer over STEPS steps inside the rank's process group; the weights after every
    sync and, with ``spy``, the checks of the module docstring."""
    import torch.distributed as dist

    import ewdml
    from ewdml.compress import oracle
    from ewdml.runtime import Trainer

    tr = Trainer(ewdml.parse_args(BASE + flags))
    ex, flat = tr.exchange, tr.flat
    inner, N = ex.inner, tr.world
    out = {"synced": [], "d_exact": [], "d_close": [], "sim_exact": [], "best": []}
    if spy:
        sim = {"anchor": ex.anchor.clone(), "data": torch.zeros_like(flat.data),
               "u": torch.zeros_like(flat.data)}
        kind, lr, mu = ex.outer
        own = {}
        begin, outer_step = inner.begin, ex._outer_step

        def spy_begin():
            if inner.src_flat:
                own["delta"] = flat.grad.clone()
            begin()

        def spy_outer():
            d = flat.grad.clone()
            inv = float(torch.tensor(1.0 / N, dtype=torch.float32))
            if inner.codec.allreduce:  # the ranks' own deltas, gathered
                rows = [torch.zeros_like(d) for _ in range(N)]
                dist.all_gather(rows, own["delta"])
                mean = sum(rows[1:], rows[0].clone()) * inv
                slack = 3 * U * sum(r.abs() for r in rows) * inv + U * d.abs()
                out["d_close"].append(bool(((d - mean).abs() <= slack).all()))
            else:  # every rank's row of the all-gather, decoded on its own
                dec = [torch.zeros_like(d) for _ in range(N)]
                for b in flat.buckets:
                    recv = inner.recv[b.index].view(N, -1)
                    for r in range(N):
                        inner.codec.decode(b.index, recv[r:r + 1],
                                           dec[r][b.start:b.start + b.length], 1.0)
                if ex.select_best:
                    best = int(ex.best_t)
                    out["best"].append(best)
                    want = dec[best]
                else:
                    want = sum(dec[1:], dec[0].clone()) * inv
                used = torch.zeros_like(d, dtype=torch.bool)  # padding keeps data - anchor = 0
                for p, o in zip(flat.params, flat.offsets):
                    used[o:o + p.numel()] = True
                out["d_exact"].append(torch.equal(_bits(d[used]), _bits(want[used]))
                                      and not bool(d[~used].any()))
            outer_step()
            oracle.outer_apply(sim["anchor"], sim["data"], sim["u"], d, lr, mu, kind == "nesterov")
            out["sim_exact"].append(
                torch.equal(_bits(ex.anchor), _bits(sim["anchor"]))
                and torch.equal(_bits(flat.data), _bits(sim["data"]))
                and torch.equal(_bits(ex.outer_momentum), _bits(sim["u"])))

        inner.begin, ex._outer_step = spy_begin, spy_outer
    for step in range(STEPS):
        tr.train_step()
        if (step + 1) % EVERY == 0:
            out["synced"].append(flat.data.clone())
    out["delta_norm"], out["momentum_norm"] = ex.outer_delta_norm, ex.outer_momentum_norm
    if ex.outer is not None:
        out["norm_ref"] = float(ex.outer_momentum.double().norm())
    tr.close()
    return out


def _many(rank, world, cases):
    return {name: _run(flags, spy) for name, flags, spy in cases}


def _replicas_identical(res, name, world):
    for k in range(STEPS // EVERY):
        for r in range(1, world):
            assert torch.equal(_bits(res[r][name]["synced"][k]), _bits(res[0][name]["synced"][k]))


@pytest.mark.parametrize("world", [2, 3])
def test_identity_setting_is_bitwise_the_run_without_the_flag(tmp_path, world):
    cases = [("plain", [], False),
             ("sgd10", ["--outer-optimizer", "sgd", "--outer-lr", "1", "--outer-momentum", "0"],
              False),
             ("plain_best", ["--select-best"], False),
             ("sgd10_best", ["--select-best", "--outer-optimizer", "sgd"], False)]
    res = run_world(_many, world, tmp_path, args=(cases,))
    for a, b in (("plain", "sgd10"), ("plain_best", "sgd10_best")):
        _replicas_identical(res, b, world)
        for r in range(world):
            for x, y in zip(res[r][a]["synced"], res[r][b]["synced"]):
                assert torch.equal(_bits(x), _bits(y))
    assert res[0]["plain"]["delta_norm"] is None
    assert res[0]["sgd10"]["delta_norm"] > 0
    # the same weights need not mean the same path: the flag's run went through the outer step
    assert abs(res[0]["sgd10"]["momentum_norm"] - res[0]["sgd10"]["norm_ref"]) \
        <= 1e-6 * res[0]["sgd10"]["norm_ref"]


@pytest.mark.parametrize("world", [2, 3])
def test_nesterov_matches_the_single_process_simulation(tmp_path, world):
    cases = [("topk", DILOCO, True),  # the default codec, with error feedback
             ("dense", DILOCO + ["--compress", "none"], True),
             ("best", DILOCO + ["--select-best"], True)]
    res = run_world(_many, world, tmp_path, args=(cases,))
    syncs = STEPS // EVERY
    for name, _, _ in cases:
        _replicas_identical(res, name, world)
        for r in range(world):
            got = res[r][name]
            assert got["sim_exact"] == [True] * syncs, (name, r)
            if name == "dense":
                assert got["d_close"] == [True] * syncs
            else:
                assert got["d_exact"] == [True] * syncs, (name, r)
    assert len(res[0]["best"]["best"]) == syncs
    assert res[0]["best"]["best"] == res[world - 1]["best"]["best"]
    # a gain of 7 over plain averaging: not the run without the flag
    plain = run_world(_many, world, tmp_path / "p", args=([("plain", [], False)],))
    assert not torch.equal(plain[0]["plain"]["synced"][-1], res[0]["topk"]["synced"][-1])


FIT = BASE[:BASE.index("--eval-freq")] + ["--sync-every", str(EVERY), "--sync-mode", "model",
                                           "--select-best"]


def _fit(rank, world, flags):
    import warnings

    import ewdml
    from ewdml.runtime import Trainer

    with warnings.catch_warnings(record=True) as seen:
        warnings.simplefilter("always")
        tr = Trainer(ewdml.parse_args(FIT + flags))
        tr.fit()
    om = tr.exchange.outer_momentum
    return {"params": tr.flat.data.clone(), "mom": tr.opt.mom.clone(), "step": tr.step,
            "outer": None if om is None else om.clone(), "anchor": tr.exchange.anchor.clone(),
            "warned": [str(w.message) for w in seen if "outer_momentum" in str(w.message)]}


def test_checkpoint_without_outer_momentum_resumes_from_zeros_with_one_warning(tmp_path):
    d = str(tmp_path / "ck") + "/"
    run_world(_fit, 2, tmp_path / "a", args=(["--max-steps", "5", "--eval-freq", "5",
                                              "--train-dir", d],))
    res = run_world(_fit, 2, tmp_path / "b", args=(DILOCO + ["--max-steps", "5", "--eval-freq",
                                                             "0", "--resume", "--train-dir", d],))
    assert len(res[0]["warned"]) == 1 and "starts from zeros" in res[0]["warned"][0]
    assert res[1]["warned"] == []
    assert all(float(res[r]["outer"].abs().max()) == 0 and res[r]["step"] == 5 for r in (0, 1))


def test_resume_between_two_syncs_reproduces_the_uninterrupted_run(tmp_path):
    """Checkpoint at step 5, between the syncs of steps 3 and 6: the shared outer momentum comes
    back next to the anchor, so the resumed run is the uninterrupted one bit for bit."""
    full = run_world(_fit, 2, tmp_path / "a", args=(DILOCO + ["--max-steps", "9", "--eval-freq",
                                                              "0", "--train-dir",
                                                              str(tmp_path / "ca") + "/"],))
    d = str(tmp_path / "cb") + "/"
    run_world(_fit, 2, tmp_path / "b", args=(DILOCO + ["--max-steps", "5", "--eval-freq", "5",
                                                       "--train-dir", d],))
    res = run_world(_fit, 2, tmp_path / "c", args=(DILOCO + ["--max-steps", "9", "--eval-freq",
                                                             "0", "--resume", "--train-dir", d],))
    assert float(full[0]["outer"].abs().max()) > 0
    for r in (0, 1):
        assert res[r]["step"] == 9 and res[r]["warned"] == []
        for k in ("params", "mom", "outer", "anchor"):
            assert torch.equal(_bits(res[r][k]), _bits(full[r][k])), k
    from ewdml.utils import checkpoint as ckpt

    st = ckpt.load(ckpt.latest(d))
    assert st["extra"]["outer_momentum"].shape == full[0]["outer"].shape
    del st
