"""Gradient clipping and EMA weights under data parallelism: two ranks (gloo rendezvous, both on the box's single GPU, started as
fresh child processes like tests/test_ddp_gpu.py) train three steps; tests/helpers/optim_ext_ddp_worker.py says what each of its
three result lines holds.  The worker runs once for the three tests."""
import functools
import os
import socket
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@functools.lru_cache(maxsize=None)
def worker_lines():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", OMP_NUM_THREADS="2")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
           "--master-port", str(port), os.path.join(ROOT, "tests", "helpers", "optim_ext_ddp_worker.py")]
    r = subprocess.run(cmd, env=env, cwd=ROOT, capture_output=True, text=True, timeout=600)
    lines = {l.split()[0]: l for l in r.stdout.splitlines() if l.startswith("OPTIM_EXT_DDP_")}
    assert r.returncode == 0 and len(lines) == 3, (r.stdout[-2000:], r.stderr[-3000:])
    return lines


def check(tag):
    line = worker_lines()[tag]
    print(line)                                  # the figures, whether or not they pass
    assert " ok=1 " in line, line


def test_replicas_stay_bit_identical():
    """weight arena, EMA arena and every step's last_grad_norm after three clipped steps: the same bits on both ranks"""
    check("OPTIM_EXT_DDP_RANKS")


def test_each_step_matches_the_single_process_replay():
    """tests/test_ddp_gpu.py's parity check (one step from a common state, 1e-5 per tensor) at each of the three steps: gradient
    arena, weights, EMA weights and the norm.  Measured on an MI355X: gradients <= 1.8e-6, weights and EMA <= 4.3e-8, norm equal."""
    check("OPTIM_EXT_DDP_STEP")


def test_three_free_running_steps_match_the_single_process_replay():
    """The same replay left to run the three steps on its own state: weights, EMA weights and every step's norm after step 3 against
    DDP's, within the 1e-5 per tensor of tests/test_ddp_gpu.py.  Measured on an MI355X: weights 4.3e-8, EMA 3.9e-8, norms equal.

    The figure needs a problem that does not amplify rounding, so the worker uses the state, batch and tile size of the
    project's own three-step comparison (tests/test_hip_modules.py::test_train_steps_match_oracle: synthetic state, bn3 damped,
    6 x 81 x 81 per BatchNorm batch).  On a randomly initialised network at 4 x 65 x 65 per rank the same comparison measured
    5.6e-2 (weights), 5.2e-2 (EMA) and 1.2e-3 (norm) while each step replayed from a common state agreed to 3.2e-6: weights a
    few ulps apart after step 1 gave step-2 gradients 0.22 of a tensor's scale apart -- the network's conditioning
    (test_train_steps_undamped_vs_float64), which no fp32 step can repair."""
    check("OPTIM_EXT_DDP_FREE")
