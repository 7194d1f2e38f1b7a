"""examples/ex_eigs_dhip_amg.c from plain C: LUNDA.mtx with the Jacobi and with the aggregation algebraic multigrid
preconditioner; the program returns 0 (both solves converged, to the same eigenvalues) and both outer-iteration counts parse."""
import os
import re
import subprocess

import pytest

import amg_cases as AMG

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_c_example_amg(built):
    exe = os.path.join(ROOT, "examples", "ex_eigs_dhip_amg")
    if not os.path.exists(exe):
        subprocess.check_call(["make", "-C", os.path.join(ROOT, "examples")])
    out = subprocess.run([exe, AMG.LUNDA], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300)
    assert out.returncode == 0, out.stdout[-2000:]
    jac = int(re.search(r"with the Jacobi preconditioner: (\d+)", out.stdout).group(1))
    amg = int(re.search(r"with the algebraic multigrid preconditioner: (\d+)", out.stdout).group(1))
    levels = int(re.search(r"on (\d+) levels", out.stdout).group(1))
    print(f"LUNDA.mtx from C: outer iterations {jac} with Jacobi, {amg} with AMG on {levels} levels")
    assert jac > 0 and amg > 0 and levels == 1
