"""Counting passes of the thresh encode's threshold search in steady state.

Trains ``--network`` with ``--compress thresh`` in eager steps, and from step ``--skip`` on hands
every encode a per-chunk counter (``ops.thresh_encode(passes=...)``, a debug output the trainer
never asks for).  Prints one JSON line: the mean, the median and the largest number of passes per
chunk row and step, and the share of chunk rows that needed one pass.

    python -m tools.probes.thresh_probe --network VGG11 --dataset Cifar10 --steps 40 --skip 10
"""
import argparse
import json

import torch


def main(argv=None):
    p = argparse.ArgumentParser()
    p.add_argument("--network", default="LeNet")
    p.add_argument("--dataset", default="MNIST")
    p.add_argument("--batch-size", type=int, default=64)
    p.add_argument("--topk-ratio", type=float, default=0.01)
    p.add_argument("--steps", type=int, default=40)
    p.add_argument("--skip", type=int, default=10, help="steps before the counting starts")
    a = p.parse_args(argv)

    import ewdml
    from ewdml import ops
    from ewdml.runtime import Trainer

    torch.manual_seed(0)
    tr = Trainer(ewdml.parse_args([
        "--network", a.network, "--dataset", a.dataset, "--batch-size", str(a.batch_size),
        "--synthetic-size", str(max(4096, 8 * a.batch_size)), "--compress", "thresh",
        "--topk-ratio", str(a.topk_ratio), "--lr", "0.01", "--momentum", "0.9", "--eval-freq",
        "0", "--quiet", "--device", "cuda", "--hip-graph", "off", "--max-steps", str(a.steps)]))
    encode = ops.thresh_encode
    counters, seen = {}, []

    def counted(dp, grad, payload, layout, resid=None, state=None, passes=None):
        buf = counters.setdefault(id(dp), torch.zeros(dp.plan.num_chunks, dtype=torch.int32,
                                                      device=payload.device))
        encode(dp, grad, payload, layout, resid=resid, state=state, passes=buf)
        seen.append(buf.clone())

    for step in range(a.steps):
        if step == a.skip:
            ops.thresh_encode = counted
        tr.train_step()
    torch.cuda.synchronize()
    ops.thresh_encode = encode
    tr.close()
    n = torch.cat(seen).float().cpu()
    print(json.dumps({"probe": "thresh_passes", "network": a.network, "ratio": a.topk_ratio,
                      "steps_counted": a.steps - a.skip, "chunk_encodes": int(n.numel()),
                      "mean_passes": round(float(n.mean()), 3),
                      "median_passes": float(n.median()), "max_passes": int(n.max()),
                      "one_pass_share": round(float((n == 1).float().mean()), 3)}))


if __name__ == "__main__":
    main()
