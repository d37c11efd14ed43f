"""Times of local SGD's sync-step tail on one GPU, with and without an outer optimizer.

Two figures per setting (none | sgd 1/0 | nesterov 0.7/0.9), one JSON line each:

* ``tail_us``: the tail alone on buffers of ``--numel`` elements -- the four torch passes of the
  run without the flag (scale into grad, add, copy, and the bf16 shadow when ``--shadow``) or the
  one ``k_outer_apply`` launch -- the median over ``--reps`` launches, HIP events around each;
* ``sync_ms`` / ``local_ms``: the trainer's captured sync and local steps (``--network``, Method 6
  with ``--sync-every 2``), the median over ``--steps`` steps of each kind.

    python -m tools.probes.outer_probe [--numel N] [--network VGG11] [--out FILE]
"""
import argparse
import json
import statistics
import sys

import torch

SETTINGS = {"none": None, "sgd_1_0": ("sgd", 1.0, 0.0), "nesterov_0.7_0.9": ("nesterov", 0.7, 0.9)}


def _timed(fn, reps):
    out = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b) * 1e3)
    return statistics.median(out)


def tail_us(setting, numel, shadow, reps):
    from ewdml import ops

    dev = "cuda"
    anchor, data, mom, grad = (torch.randn(numel, device=dev) for _ in range(4))
    mom.mul_(0.01)
    grad.mul_(0.01)
    sh = torch.zeros(numel, dtype=torch.bfloat16, device=dev) if shadow else None
    stats = torch.zeros((ops.outer_rows(numel), 2), device=dev)
    if setting is None:
        def fn():
            grad.mul_(1.0)  # the dense decode's own write
            torch.add(anchor, grad, out=data)
            anchor.copy_(data)
            if sh is not None:
                sh.copy_(data)
    else:
        kind, lr, mu = setting

        def fn():
            grad.mul_(1.0)
            ops.outer_apply(anchor, data, mom, grad, lr, mu, kind == "nesterov", shadow=sh,
                            stats=stats)
    for _ in range(5):
        fn()
    g = torch.cuda.CUDAGraph()  # as in the captured sync step: no launch gaps between the passes
    with torch.cuda.graph(g):
        fn()
    return _timed(g.replay, reps)


def step_ms(setting, network, steps):
    import ewdml
    from ewdml.runtime import Trainer

    flags = ["--network", network, "--dataset", "MNIST" if network == "LeNet" else "Cifar10",
             "--batch-size", "128", "--synthetic-size", "4096", "--eval-freq", "0", "--quiet",
             "--device", "cuda", "--method", "6", "--sync-every", "2", "--ef-warmup", "none",
             "--momentum", "0.9", "--lr", "0.01", "--max-steps", "100000"]
    if setting is not None:
        flags += ["--outer-optimizer", setting[0], "--outer-lr", str(setting[1]),
                  "--outer-momentum", str(setting[2])]
    tr = Trainer(ewdml.parse_args(flags))
    for _ in range(8):
        tr.train_step()
    torch.cuda.synchronize()
    times = {"local": [], "sync": []}
    for _ in range(2 * steps):
        kind = "sync" if tr.exchange.is_sync else "local"
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        tr.train_step()
        b.record()
        b.synchronize()
        times[kind].append(a.elapsed_time(b))
    mode, caps = tr.graph_mode, tr.captures
    tr.close()
    return statistics.median(times["local"]), statistics.median(times["sync"]), mode, caps


def main(argv=None):
    p = argparse.ArgumentParser()
    p.add_argument("--numel", type=int, default=9756426 + 6)  # VGG-11-BN's flat buffer
    p.add_argument("--shadow", action="store_true")
    p.add_argument("--reps", type=int, default=200)
    p.add_argument("--network", default="VGG11")
    p.add_argument("--steps", type=int, default=40)
    p.add_argument("--out", default=None)
    a = p.parse_args(argv)
    a.numel -= a.numel % 4
    lines = []
    for name, setting in SETTINGS.items():
        rec = {"probe": "outer", "setting": name, "numel": a.numel, "shadow": a.shadow,
               "tail_us": round(tail_us(setting, a.numel, a.shadow, a.reps), 2)}
        local, sync, mode, caps = step_ms(setting, a.network, a.steps)
        rec.update(network=a.network, local_ms=round(local, 4), sync_ms=round(sync, 4),
                   hip_graph=mode, captures=caps)
        lines.append(json.dumps(rec))
        print(lines[-1], flush=True)
    if a.out:
        with open(a.out, "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    sys.exit(main())
