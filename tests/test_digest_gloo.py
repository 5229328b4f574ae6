"""CPU: the replica check (model_tool/parallel.py: check_replicas; --check_weights) with two ranks over gloo -- started as
tests/test_ddp_gloo.py starts its worker.  tests/digest_worker.py holds the assertions."""
import os
import socket
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _free_port():
    with socket.socket(socket.AF_INET, socket.SOCK_STREAM) as sk:
        sk.bind(("127.0.0.1", 0))
        return sk.getsockname()[1]


def test_two_ranks_agree_until_one_weight_moves_by_an_ulp(tmp_path):
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", OMP_NUM_THREADS="2")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=2",
           "--master-addr", "127.0.0.1", "--master-port", str(_free_port()), os.path.join(ROOT, "tests", "digest_worker.py")]
    out = subprocess.run(cmd, env=env, cwd=str(tmp_path), capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout[-3000:] + out.stderr[-3000:]
    assert "DIGEST_OK rank 0" in out.stdout and "DIGEST_OK rank 1" in out.stdout
    assert "weight check: 3 checks, ranks agree" in out.stdout
