"""examples/ex_eigs_dhip_amg_reuse.c: the hierarchy handle from plain C on the four tiles of LUNDA.mtx (588 rows, two levels):
one hierarchy built with the device set-up, two solves with other numEvals and another smoother attached to it.  The program
returns 0 (both solves converged, their common eigenvalues agree), prints the set-up once and both iteration counts."""
import os
import re
import subprocess

import pytest

import amg_cases as AMG

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_c_example_amg_reuse(built):
    exe = os.path.join(ROOT, "examples", "ex_eigs_dhip_amg_reuse")
    out = subprocess.run([exe, AMG.LUNDA, "4"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300)
    assert out.returncode == 0, out.stdout[-2000:]
    assert len(re.findall(r"hierarchy set-up:", out.stdout)) == 1
    m = re.search(r"hierarchy set-up: ([0-9.]+) seconds \(([0-9.]+) in the device stages\), 2 levels, rows 588 64, 0 levels built on the host", out.stdout)
    assert m and float(m.group(1)) >= float(m.group(2)) > 0.0, out.stdout[-2000:]
    assert len(re.findall(r"hip_dprimme returned 0", out.stdout)) == 2
    first = int(re.search(r"outer iterations of the first solve: (\d+)", out.stdout).group(1))
    second = int(re.search(r"outer iterations of the second solve: (\d+)", out.stdout).group(1))
    print(f"LUNDA.mtx x 4 from C: set-up {m.group(1)} s ({m.group(2)} s on the device), outer iterations {first} and {second}")
    assert first > 0 and second > 0 and "the hierarchy was attached 2 times" in out.stdout
    bad = subprocess.run([exe, AMG.LUNDA, "0"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=60)
    assert bad.returncode == 2 and "usage" in bad.stdout
