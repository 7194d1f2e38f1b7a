"""examples/ex_eigs_dhip_mg.c from plain C: the 5-point Laplacian on 63 x 65 without and with the geometric multigrid
preconditioner; the program returns 0 and the second outer-iteration count is the smaller one."""
import os
import re
import subprocess

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_c_example_mg(built):
    exe = os.path.join(ROOT, "examples", "ex_eigs_dhip_mg")
    if not os.path.exists(exe):
        subprocess.check_call(["make", "-C", os.path.join(ROOT, "examples")])
    out = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300)
    assert out.returncode == 0, out.stdout[-2000:]
    plain = int(re.search(r"without preconditioner: (\d+)", out.stdout).group(1))
    pre = int(re.search(r"with the multigrid preconditioner: (\d+)", out.stdout).group(1))
    assert pre < plain, out.stdout
