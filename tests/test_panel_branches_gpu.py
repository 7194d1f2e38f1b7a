"""Every dispatch branch of the real panel and Ritz kernels at small sizes (-m gpu): the cases of
tests/panel_branch_cases.py on the device against the longdouble references written from the header's contract, with the
derived bounds and the guard / padding comparison of every operand.  One test per (entry point, type, alignment, flag);
its cases run on one context.  The same cases run on the plain-C oracle in tests/test_panel_branches_host.py, which also
asserts that the tables cover every instantiation.

Run as a script (`python tests/test_panel_branches_gpu.py wide`) this file is the child process of
test_dots_wide_kernel_without_matrix_cores: HIPK_NO_MFMA is read once per process."""
import os
import subprocess
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
if __name__ == "__main__":
    ROOT = os.path.dirname(HERE)
    sys.path[:0] = [ROOT, os.path.join(ROOT, "oracle"), HERE]

from kernel_harness import Dev
import panel_branch_cases as P

pytestmark = pytest.mark.gpu

TABLES = ["residual", "residual_dev", "project", "project_mul", "dots", "ritz_update", "update_overlaps", "triple"]
GROUPS = P.groups(TABLES)


@pytest.mark.parametrize("gid,cases", GROUPS, ids=[g for g, _ in GROUPS])
def test_device_against_longdouble_reference(built, gid, cases):
    rep = P.run_cases(Dev, cases)
    print(f"{gid}: {rep.summary()}")
    assert not rep.fails, f"{gid}: {rep.summary()}\n" + "\n".join(rep.fails[:20])


def test_dots_wide_kernel_without_matrix_cores(built):
    """dots_wide_kernel serves blocks of >= 4 right-hand columns on aligned panels only when HIPK_NO_MFMA is set, and the
    knob is read once per process: one fresh child runs those cases against the same references"""
    env = dict(os.environ, HIPK_NO_MFMA="1")
    p = subprocess.run([sys.executable, os.path.abspath(__file__), "wide"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True,
                       env=env, timeout=120)
    print(p.stdout[-2000:])
    assert p.returncode == 0 and "dots_wide: ok" in p.stdout, p.stdout[-4000:]


if __name__ == "__main__":
    assert sys.argv[1:] == ["wide"] and os.environ.get("HIPK_NO_MFMA")
    cases = P.CASES["dots_wide"]
    assert all(P.branch_of(c)[0] == "dots_wide_kernel" for c in cases)
    rep = P.run_cases(Dev, cases)
    print(f"dots_wide: {rep.summary()}")
    if rep.fails:
        print("\n".join(rep.fails[:20]))
        sys.exit(1)
    print("dots_wide: ok")
