"""LARS and LAMB through the trainer on CPU/Gloo: 2 and 3 ranks train LeNet for 4 steps over the
dense all-reduce and the sign codec; the replicas stay bitwise identical and equal a
single-process optimizer fed the averaged gradients the exchange produced, and a checkpoint
taken after step 2 resumes bit for bit."""
import pytest
import torch

from .helpers import run_world

pytestmark = pytest.mark.slow

STEPS = 4
BASE = ["--network", "LeNet", "--dataset", "MNIST", "--batch-size", "16", "--synthetic-size",
        "512", "--eval-freq", "0", "--quiet", "--device", "cpu", "--log-interval", "1000",
        "--weight-decay", "0.0005", "--no-legacy-ckpt", "--bucket-mb", "0.25"]
OPT = {"lamb": ["--optimizer", "lamb", "--lr", "0.002"],
       "lars": ["--optimizer", "lars", "--lr", "0.5", "--momentum", "0.9", "--lars-eta", "0.01"]}


def _bits(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32),
                                              b.contiguous().view(torch.int32))


def _opt_state(opt):
    return {k: v.clone() for k, v in opt.state_dict().items() if torch.is_tensor(v)}


def _train(rank, world, opt, compress, ckpt_dir, stop_at, resume):
    """Steps up to ``stop_at`` (checkpoint there), or -- ``resume`` -- from the checkpoint on.
    Records every gradient range the exchange hands to the optimizer."""
    import ewdml
    from ewdml.runtime import Trainer

    args = BASE + OPT[opt] + ["--compress", compress, "--max-steps", str(STEPS), "--train-dir",
                              ckpt_dir]
    tr = Trainer(ewdml.parse_args(args + (["--resume"] if resume else [])))
    out = {"start": tr.step, "before": tr.flat.data.clone(), "fed": [], "nb": len(tr.flat.buckets)}
    real = tr.opt.step_range

    def step_range(start, length, grad, grad_scale=1.0):
        out["fed"].append((tr.opt.steps, start, length, grad.clone(), grad_scale))
        real(start, length, grad, grad_scale)

    tr.opt.step_range = step_range
    while tr.step < stop_at:
        tr.train_step()
    out["params"] = tr.flat.data.clone()
    out["opt"] = _opt_state(tr.opt)
    out["resid"] = tr.exchange.resid.clone() if getattr(tr.exchange, "resid", None) is not None \
        else None
    if stop_at < STEPS:
        tr.save_checkpoint()
    tr.close()
    return out


def _replay(opt, r0):
    """A single-process optimizer over the same LeNet start, fed whole-model gradients assembled
    from the ranges rank 0's exchange handed over."""
    import ewdml
    from ewdml.models import build_model
    from ewdml.optim import make_optimizer
    from ewdml.parallel.flat import FlatModel

    cfg = ewdml.parse_args(BASE + OPT[opt])
    flat = FlatModel(build_model("LeNet", 10), bucket_bytes=1 << 30)
    assert len(flat.buckets) == 1 and flat.numel == r0["before"].numel()
    flat.data.copy_(r0["before"])
    single = make_optimizer(opt, flat, lr=cfg.lr, momentum=cfg.momentum,
                            weight_decay=cfg.weight_decay, eta=cfg.lars_eta, eps=cfg.adam_eps)
    for s in range(STEPS):
        g = torch.zeros(flat.numel)
        scales = set()
        for step, start, length, grad, scale in r0["fed"]:
            if step == s:
                g[start:start + length] = grad.float()
                scales.add(scale)
        assert len(scales) == 1
        single.step(grad=g, grad_scale=scales.pop())
    return flat, single


@pytest.mark.parametrize("compress", ["none", "sign"])
@pytest.mark.parametrize("opt", ["lamb", "lars"])
@pytest.mark.parametrize("world", [2, 3])
def test_replicas_identical_and_equal_one_process(tmp_path, world, opt, compress):
    res = run_world(_train, world, tmp_path, args=(opt, compress, str(tmp_path / "ck"), STEPS,
                                                   False))
    r0 = res[0]
    assert r0["nb"] >= 2 and not _bits(r0["params"], r0["before"])
    for r in res[1:]:
        assert _bits(r["params"], r0["params"])
        for k, v in r["opt"].items():
            assert _bits(v, r0["opt"][k]), k
    if compress == "sign":
        assert all(float(r["resid"].abs().max()) > 0 for r in res)
        assert not torch.equal(res[1]["resid"], r0["resid"])  # per-rank state
    threads = torch.get_num_threads()
    torch.set_num_threads(1)  # as the ranks ran: torch's CPU sums depend on the thread count
    try:
        flat, single = _replay(opt, r0)
    finally:
        torch.set_num_threads(threads)
    assert _bits(flat.data, r0["params"])
    for k, v in _opt_state(single).items():
        assert _bits(v, r0["opt"][k]), k
    ratio = r0["opt"]["ratio"]
    assert float(ratio.min()) > 0 and bool((ratio != 1).any())


@pytest.mark.parametrize("opt,compress", [("lamb", "sign"), ("lars", "none")])
def test_resume_after_step_two_is_bit_exact(tmp_path, opt, compress):
    world = 2
    full = run_world(_train, world, tmp_path / "a", args=(opt, compress, str(tmp_path / "a" / "ck"),
                                                          STEPS, False))
    ck = str(tmp_path / "b" / "ck")
    run_world(_train, world, tmp_path / "b1", args=(opt, compress, ck, 2, False))
    rest = run_world(_train, world, tmp_path / "b2", args=(opt, compress, ck, STEPS, True))
    for r, f in zip(rest, full):
        assert r["start"] == 2
        assert [s[0] for s in r["fed"]][0] == 2  # the step counter came back
        assert _bits(r["params"], f["params"])
        for k, v in r["opt"].items():
            assert _bits(v, f["opt"][k]), k
        if compress == "sign":
            assert _bits(r["resid"], f["resid"])
