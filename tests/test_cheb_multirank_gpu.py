"""Two ranks sharing one GPU: the row-partitioned 60 x 61 Laplacian with the Chebyshev polynomial preconditioner (generic
path: operator with halo exchange + update kernel) reproduces the one-rank solve."""
import json
import os
import socket
import subprocess
import sys

import numpy as np
import pytest

import cheb_cases as CC

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))


def test_two_ranks_reproduce_one_rank(built, tmp_path):
    one = CC.run_case("gdk_60x61_s8", "hip")
    assert one.ret == 0
    s = socket.socket(); s.bind(("127.0.0.1", 0)); port = s.getsockname()[1]; s.close()
    out = str(tmp_path / "res_cheb")
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0", PRIMME_AMD_COMM="ipc", PRIMME_AMD_IPC_DEVICE_TIMEOUT_S="120")
    procs = [subprocess.Popen([sys.executable, os.path.join(HERE, "mp_worker_cheb_gpu.py"), str(r), "2", str(port), out],
                              stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, env=env) for r in range(2)]
    outs = []
    try:
        outs = [p.communicate(timeout=600)[0] for p in procs]
    finally:
        for p in procs:
            if p.poll() is None:
                p.kill()
    assert all(p.returncode == 0 for p in procs), "\n".join(o[-1500:] for o in outs)
    res = [json.load(open(f"{out}.{r}")) for r in range(2)]
    for r in res:
        assert r["ret"] == 0
        assert np.max(np.abs(np.array(r["evals"]) - one.evals)) <= 1e-10 * 8.0
        assert np.all(np.array(r["resNorms"]) <= 1e-8 * 8.0 * (1 + 1e-6))
        its = one.stats["numOuterIterations"]
        assert abs(r["its"] - its) <= max(2, 0.02 * its), (r["its"], its)
        assert r["stats"]["fused_steps"] == 0 and r["stats"]["operator_products"] == 7 * r["stats"]["applies"]
        assert r["gershgorin"] == [0.0, 8.0]
