"""A/B of the optimizer step alone: ``ops.adam8_step`` (8-bit Adam, ``FlatAdam8bit``) against
``ops.adam_flat`` (``FlatAdam``) over the VGG-11 preset's flat buffer, fp32 gradients.

Every timed region is ``--launches`` whole-model steps (replays of a captured graph of 30)
between two device events; the two optimizers alternate within a round, ``--rounds`` rounds after
a warm-up of each.  Each optimizer
steps ``--copies`` separate models in turn so that a region's working set (28 B resp. 16 B per
element and copy) exceeds the 256 MB last-level cache and every launch reads HBM, as a step
between a backward and a forward pass does.  Prints one line per region, then the medians, the
spread and the achieved bytes/s (bytes the algorithm needs: 8 parameter + 4 gradient + 16 resp.
4 + 16/256 state bytes per element)."""
import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))

from ewdml.models import build_model  # noqa: E402
from ewdml.optim import FlatAdam, FlatAdam8bit  # noqa: E402
from ewdml.parallel.flat import FlatModel  # noqa: E402

GRAPH = 30  # steps per captured graph


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--network", default="VGG11")
    ap.add_argument("--launches", type=int, default=2400)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--copies", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "this A/B needs a GPU"
    torch.manual_seed(0)
    sets = {"adam": [], "adam8bit": []}
    for name, cls in (("adam", FlatAdam), ("adam8bit", FlatAdam8bit)):
        for _ in range(a.copies):
            flat = FlatModel(build_model(a.network).cuda())
            for o, p in zip(flat.offsets, flat.params):
                flat.grad[o:o + p.numel()].normal_(0.0, 0.01)
            sets[name].append(cls(flat, lr=1e-4))
    n = sets["adam"][0].flat.param_numel
    need = {"adam": 28.0 * n, "adam8bit": (16.0 + 16.0 / 256.0) * n}

    def steps(name, launches):
        opts = sets[name]
        for i in range(launches):
            o = opts[i % len(opts)]
            o.step_range(0, o.flat.numel, o.flat.grad)  # no end_step: the step kernel alone

    # one captured graph of GRAPH steps per optimizer, so that a region times the kernels and not
    # the Python that enqueues them
    graphs = {}
    for name in sets:
        steps(name, GRAPH)  # warm-up: code objects, plans
        torch.cuda.synchronize()
        graphs[name] = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graphs[name]):
            steps(name, GRAPH)

    def region(name, launches):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(launches // GRAPH):
            graphs[name].replay()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) * 1e3 / (launches // GRAPH * GRAPH)  # us per step

    lines = [f"# {a.network}: {n} parameters, flat {sets['adam'][0].flat.numel} elements, "
             f"{a.copies} copies, {a.launches} launches per region, {a.rounds} rounds"]
    for name in sets:
        region(name, 10 * GRAPH)
    times = {k: [] for k in sets}
    for r in range(a.rounds):
        for name in sets:
            us = region(name, a.launches)
            times[name].append(us)
            lines.append(f"round {r} {name} {us:.2f} us/step {need[name] / us * 1e-6:.3f} TB/s")
    for name, ts in times.items():
        med = statistics.median(ts)
        lines.append(f"{name}: median {med:.2f} us min {min(ts):.2f} max {max(ts):.2f} "
                     f"({need[name] / 1e6:.1f} MB needed, {need[name] / med * 1e-6:.3f} TB/s)")
    lines.append(f"adam / adam8bit median ratio "
                 f"{statistics.median(times['adam']) / statistics.median(times['adam8bit']):.3f}")
    print("\n".join(lines))
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
