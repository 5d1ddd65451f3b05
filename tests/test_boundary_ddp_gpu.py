"""The boundary criterion under data parallelism, as tests/test_distill_ddp_gpu.py runs the distillation one: two ranks (gloo
rendezvous, both on the box's single GPU), each with half of a batch of 4, one half all ignored -- see
tests/helpers/boundary_ddp_worker.py for what is asserted."""
import os
import socket
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_two_ranks_form_the_global_batch_loss_gradient_and_count():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", OMP_NUM_THREADS="2")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
           "--master-port", str(port), os.path.join(ROOT, "tests", "helpers", "boundary_ddp_worker.py")]
    r = subprocess.run(cmd, env=env, cwd=ROOT, capture_output=True, text=True, timeout=600)
    line = [l for l in r.stdout.splitlines() if l.startswith("BOUNDARY_DDP")]
    assert r.returncode == 0 and line, (r.stdout[-2000:], r.stderr[-3000:])
    print(line[0])
