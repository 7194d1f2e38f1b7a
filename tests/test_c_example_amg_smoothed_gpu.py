"""examples/ex_eigs_dhip_amg.c with --smoothed: primme_amd_operator_set_amg_smoothed from plain C on LUNDA.mtx (one level, so
the hierarchy is the dense inverse either way: the switch, the entry point and the counters are what this checks); the program
returns 0 and names the smoothed solve.  Another second argument is a usage error."""
import os
import re
import subprocess

import pytest

import amg_cases as AMG

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_c_example_amg_smoothed(built):
    exe = os.path.join(ROOT, "examples", "ex_eigs_dhip_amg")
    out = subprocess.run([exe, AMG.LUNDA, "--smoothed"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300)
    assert out.returncode == 0, out.stdout[-2000:]
    assert "amg (smoothed): hip_dprimme returned 0" in out.stdout
    jac = int(re.search(r"with the Jacobi preconditioner: (\d+)", out.stdout).group(1))
    amg = int(re.search(r"with the algebraic multigrid preconditioner: (\d+)", out.stdout).group(1))
    print(f"LUNDA.mtx from C: outer iterations {jac} with Jacobi, {amg} with smoothed AMG")
    assert 0 < amg < jac
    bad = subprocess.run([exe, AMG.LUNDA, "--smooth"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=60)
    assert bad.returncode == 2 and "usage" in bad.stdout
