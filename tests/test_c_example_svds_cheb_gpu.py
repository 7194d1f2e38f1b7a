"""examples/ex_svds_dhip_cheb.c from plain C: the smallest singular values of the difference matrix without and with the
Chebyshev polynomial preconditioner; the program returns 0 and the second outer-iteration count is the smaller one."""
import os
import re
import subprocess

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_c_example_svds_cheb(built):
    exe = os.path.join(ROOT, "examples", "ex_svds_dhip_cheb")
    if not os.path.exists(exe):
        subprocess.check_call(["make", "-C", os.path.join(ROOT, "examples")])
    out = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300)
    assert out.returncode == 0, out.stdout[-2000:]
    plain = int(re.search(r"without preconditioner: (\d+)", out.stdout).group(1))
    pre = int(re.search(r"with the Chebyshev preconditioner: (\d+)", out.stdout).group(1))
    assert pre < plain, out.stdout
