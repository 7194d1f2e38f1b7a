"""Every dispatch branch of the CSR row-tile product kernels at small sizes (-m gpu): the cases of tests/csr_branch_cases.py
on the device against the longdouble references written from the header's contract, with the derived per-row bounds, the
guard / padding comparison of every operand and the bit-for-bit repeat of every product.  One test per (entry point, type,
flavour); its cases run on one context.  The same cases run on the plain-C oracle in tests/test_csr_branches_host.py, which
also asserts that the tables cover every instantiation and every reachable per-tile cell.

The instantiations and paths that only an environment knob selects (csr_knobs() reads the environment once per process)
run in one fresh child process per knob set: this file run as a script, `python tests/test_csr_branches_gpu.py <knob set>`."""
import os
import subprocess
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
if __name__ == "__main__":
    ROOT = os.path.dirname(HERE)
    sys.path[:0] = [ROOT, os.path.join(ROOT, "oracle"), HERE]

from kernel_harness import Dev
import csr_branch_cases as B

pytestmark = pytest.mark.gpu

GROUPS = B.groups()
KNOB_SETS = [k for k in B.KNOBS if k]


@pytest.mark.parametrize("gid,cases", GROUPS, ids=[g for g, _ in GROUPS])
def test_device_against_longdouble_reference(built, gid, cases):
    rep = B.run_cases(Dev, cases)
    print(f"{gid}: {rep.summary()}")
    assert not rep.fails, f"{gid}: {rep.summary()}\n" + "\n".join(rep.fails[:20])


@pytest.mark.parametrize("knobs", KNOB_SETS)
def test_knob_variants_in_a_fresh_process(built, knobs):
    """one child at a time, the knob set in its environment; the child checks through branch_of that its cases land in the
    instantiations it is there for, runs them against the same references and bounds, and prints `<knob set>: ok`"""
    env = dict(os.environ, **B.KNOBS[knobs]["env"])
    p = subprocess.run([sys.executable, os.path.abspath(__file__), knobs], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True,
                       env=env, timeout=120)
    print(p.stdout[-2000:])
    assert p.returncode == 0 and f"{knobs}: ok" in p.stdout, p.stdout[-4000:]


if __name__ == "__main__":
    assert len(sys.argv) == 2 and sys.argv[1] in KNOB_SETS
    knobs = sys.argv[1]
    assert all(os.environ.get(k) == v for k, v in B.KNOBS[knobs]["env"].items())
    B.check_knob_cases(knobs)
    failed = False
    for gid, cases in B.groups(knobs=True):
        if not gid.startswith(f"knob-{knobs}-"):
            continue
        rep = B.run_cases(Dev, cases)
        print(f"{gid}: {rep.summary()}")
        if rep.fails:
            print("\n".join(rep.fails[:20]))
            failed = True
    if failed:
        sys.exit(1)
    print(f"{knobs}: ok")
