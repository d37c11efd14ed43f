"""Graph captures of the trainer run with Python's cyclic collector off (``_no_gc`` in
runtime/trainer.py): finalizers of objects that died earlier must not run inside a stream capture.
Also prints whether a closed trainer's HIP graph is freed by reference count or only by the
collector (a fact recorded in profiles/validation/layerwise.md, not asserted)."""
import gc
import weakref

import pytest
import torch

import ewdml
from ewdml import ops

pytestmark = pytest.mark.gpu

LENET = ["--network", "LeNet", "--dataset", "MNIST", "--batch-size", "16", "--synthetic-size",
         "256", "--momentum", "0.9", "--lr", "0.01", "--eval-freq", "0", "--quiet", "--device",
         "cuda", "--hip-graph", "full", "--graph-warmup", "1", "--compress", "none",
         "--max-steps", "4"]


def test_the_collector_is_off_while_a_step_is_captured():
    from ewdml.runtime import Trainer

    ops.require()
    tr = Trainer(ewdml.parse_args(LENET))
    seen, real = [], tr.forward_backward

    def forward_backward(x, y):
        seen.append((torch.cuda.is_current_stream_capturing(), gc.isenabled()))
        return real(x, y)

    tr.forward_backward = forward_backward
    for _ in range(3):
        tr.train_step()
    torch.cuda.synchronize()
    assert tr._graphs is not None and gc.isenabled()
    assert any(cap for cap, _ in seen)
    assert all(on != cap for cap, on in seen), seen  # off exactly while capturing
    graph = weakref.ref(tr._graphs[0])
    del tr.forward_backward
    tr.close()
    gc.disable()
    try:
        del tr, real, forward_backward
        print(f"closed trainer's graph alive before a collection: {graph() is not None}")
    finally:
        gc.enable()
    gc.collect()
    assert graph() is None
