"""The optimizer step alone, one optimizer per process: ``--optimizer adam | galore | apollo`` over
a preset's flat buffer, fp32 gradients.  Run it once per optimizer, each in a fresh process, and
set the printed medians side by side.

A timed region is about ``--launches`` whole-model steps (replays of a captured graph of about
30, the device step counter advancing as in training) between two device events, ``--rounds``
regions after a warm-up.  The optimizer steps several separate models in turn, as many as it takes
for parameters, gradient and state together to reach ``--working-set-mb`` (2.5 times the 256 MB
last-level cache by default), so that nothing of a model is left in the cache when its turn comes
again.  ``--state-bytes`` prints ``state_bytes()`` of the three optimizers on the CPU instead."""
import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))

from ewdml.models import build_model  # noqa: E402
from ewdml.optim import make_optimizer  # noqa: E402
from ewdml.parallel.flat import FlatModel  # noqa: E402

GRAPH = 30  # steps per captured graph, rounded to whole turns through the models


def state_bytes(opt):
    """FlatAdam keeps two moments of the whole flat buffer and has no state_bytes()."""
    return opt.state_bytes() if hasattr(opt, "state_bytes") else 8 * opt.flat.numel


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--optimizer", default="apollo", choices=["adam", "galore", "apollo"])
    ap.add_argument("--network", default="VGG11")
    ap.add_argument("--launches", type=int, default=1200)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--working-set-mb", type=float, default=640.0)
    ap.add_argument("--state-bytes", action="store_true")
    a = ap.parse_args()
    if a.state_bytes:
        flat = FlatModel(build_model(a.network))
        sizes = {k: state_bytes(make_optimizer(k, flat)) for k in ("adam", "galore", "apollo")}
        print(f"{a.network}: {flat.param_numel} parameters, state bytes {sizes}")
        return
    assert torch.cuda.is_available(), "the step time needs a GPU"
    torch.manual_seed(0)
    opts = []
    while not opts or len(opts) * (8 * opts[0].flat.numel + state_bytes(opts[0])) < \
            a.working_set_mb * 1e6:
        flat = FlatModel(build_model(a.network).cuda())
        for o, p in zip(flat.offsets, flat.params):
            flat.grad[o:o + p.numel()].normal_(0.0, 0.01)
        opts.append(make_optimizer(a.optimizer, flat, lr=1e-4))
    glen = len(opts) * max(1, round(GRAPH / len(opts)))

    def steps():
        for i in range(glen):
            opts[i % len(opts)].step()

    steps()  # warm-up: code objects, plans
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        steps()

    def region(launches):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        replays = max(1, launches // glen)
        for _ in range(replays):
            graph.replay()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) * 1e3 / (replays * glen)  # us per step

    region(10 * glen)
    ts = [region(a.launches) for _ in range(a.rounds)]
    print(f"{a.optimizer} on {a.network}: {len(opts)} models, graph of {glen} steps, state "
          f"{state_bytes(opts[0])} B; us/step median {statistics.median(ts):.2f} min "
          f"{min(ts):.2f} max {max(ts):.2f}")


if __name__ == "__main__":
    main()
