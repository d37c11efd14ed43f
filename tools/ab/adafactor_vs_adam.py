"""A/B of the optimizer step alone: ``ops.adafactor_step`` (``FlatAdafactor``, four launches)
against ``ops.adam_flat`` (``FlatAdam``) over the VGG-11 preset's flat buffer, fp32 gradients.

Every timed region is about ``--launches`` whole-model steps (replays of a captured graph of
about 30) between two device events; the two optimizers alternate within a round, ``--rounds``
rounds after a warm-up of each.  Each optimizer steps several separate models in turn, as many as
it takes for the memory that optimizer itself touches (Adam: parameters, gradient and two moments,
16 B per element; Adafactor with no first moment: parameters and gradient, 8 B per element, plus
its state; the few MB of workspaces are not counted) to reach ``--working-set-mb``, 2.5 times the 256 MB last-level cache by
default: nothing of a model is left in the cache when its turn comes again, as a step between a
backward and a forward pass finds it.  A graph holds a whole number of turns through the models.
Prints one line per region, then the medians, the spread, both optimizers' state bytes and the
achieved bytes/s against the bytes the algorithm needs: Adam 8 parameter + 4 gradient + 16 state
bytes per element; Adafactor 8 + 4 when the gradient is read once, 8 + 12 when each of its three
passes over the gradient reads HBM."""
import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))

from ewdml.models import build_model  # noqa: E402
from ewdml.optim import FlatAdafactor, FlatAdam  # noqa: E402
from ewdml.parallel.flat import FlatModel  # noqa: E402

GRAPH = 30  # steps per captured graph, rounded to whole turns through an optimizer's models


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--network", default="VGG11")
    ap.add_argument("--launches", type=int, default=2400)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--working-set-mb", type=float, default=640.0)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "this A/B needs a GPU"
    torch.manual_seed(0)
    sets = {"adam": [], "adafactor": []}
    touched = {}  # bytes of one model that its optimizer's step reads or writes
    for name, cls in (("adam", FlatAdam), ("adafactor", FlatAdafactor)):
        while not sets[name] or len(sets[name]) * touched[name] < a.working_set_mb * 1e6:
            flat = FlatModel(build_model(a.network).cuda())
            for o, p in zip(flat.offsets, flat.params):
                flat.grad[o:o + p.numel()].normal_(0.0, 0.01)
            opt = cls(flat, lr=1e-4)
            sets[name].append(opt)
            extra = 8 * flat.numel if name == "adam" else opt.state_bytes()
            touched[name] = 8 * flat.numel + extra
    n = sets["adam"][0].flat.param_numel
    state = {"adam": 8 * sets["adam"][0].flat.numel, "adafactor": sets["adafactor"][0].state_bytes()}
    need = {"adam": 28.0 * n, "adafactor": 12.0 * n}
    glen = {k: len(v) * max(1, round(GRAPH / len(v))) for k, v in sets.items()}

    def steps(name, launches):
        opts = sets[name]
        for i in range(launches):
            o = opts[i % len(opts)]
            o.step_range(0, o.flat.numel, o.flat.grad)  # no end_step: the step kernels alone

    graphs = {}
    for name in sets:
        steps(name, glen[name])  # warm-up: code objects, plans
        torch.cuda.synchronize()
        graphs[name] = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graphs[name]):
            steps(name, glen[name])

    def region(name, launches):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        replays = max(1, launches // glen[name])
        for _ in range(replays):
            graphs[name].replay()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) * 1e3 / (replays * glen[name])  # us per step

    lines = [f"# {a.network}: {n} parameters, flat {sets['adam'][0].flat.numel} elements, "
             f"{a.launches} launches per region, {a.rounds} rounds",
             f"# state bytes: adam {state['adam']}, adafactor {state['adafactor']}"]
    for name in sets:
        lines.append(f"# {name}: {len(sets[name])} models of {touched[name] / 1e6:.1f} MB touched, "
                     f"working set {len(sets[name]) * touched[name] / 1e6:.1f} MB, "
                     f"graph of {glen[name]} steps")
        region(name, 10 * glen[name])
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
    lines.append(f"adam / adafactor median ratio "
                 f"{statistics.median(times['adam']) / statistics.median(times['adafactor']):.3f}")
    print("\n".join(lines))
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
