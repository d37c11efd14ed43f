"""bench.py with the Lion vote exchange under the multi-rank launch line, on CPU/Gloo with two
ranks (modelled on test_bench_launch.py): the JSON line, the 1-bit payload and the replica check.

bench.py spells its ``--error-feedback`` switch out on the trainer's command line either way, and
``--compress vote`` refuses an explicit ``--error-feedback`` (there is no magnitude to
compensate), so the vote runs are launched with ``--error-feedback off``."""
import json
import os
import socket
import subprocess
import sys

import pytest

pytestmark = pytest.mark.slow

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def test_bench_vote_two_ranks_gloo():
    env = dict(os.environ, CUDA_VISIBLE_DEVICES="", HIP_VISIBLE_DEVICES="")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2",
           "--master-addr", "127.0.0.1", "--master-port", str(_free_port()), "bench.py",
           "--gpus", "2", "--steps", "2", "--warmup", "1", "--preset", "lenet",
           "--batch-size", "32", "--hip-graph", "off", "--compress", "vote",
           "--error-feedback", "off", "--extra", "--optimizer lion --lr 1e-4"]
    r = subprocess.run(cmd, cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout  # rank 0 only
    rec = json.loads(lines[0])
    assert rec["n_gpus"] == 2 and rec["config"]["parallelism"] == "dp2"
    assert rec["config"]["codec"] == "vote1b" and rec["config"]["error_feedback"] is False
    assert rec["replicas_identical"] is True
    # one bit per element in 1024-byte chunk rows, and nothing else: every rank sends as much
    assert rec["payload_bytes_per_rank"] % 1024 == 0
    assert rec["grad_bytes_per_step_on_wire"] == 2 * rec["payload_bytes_per_rank"]
    assert 25 < rec["compression_ratio"] <= 32
    assert rec["value"] > 0 and rec["final_loss"] == rec["final_loss"]
