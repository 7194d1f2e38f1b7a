"""Every branch of the row-pattern, panel-blocked and stencil kernels at small sizes (-m gpu): the cases of
tests/structured_branch_cases.py on the device against the longdouble references written from the header's contract, with the
derived per-row bounds, the guard / padding comparison of every operand, the bit-for-bit repeat of every product and, for the
one-column product of the row-pattern form, bit identity with the row tiles after hipk_set_spmv_format(0).  One test per (entry
point, type, flavour); its cases run on one context.  The same cases run on the plain-C oracle in
tests/test_structured_branches_host.py, which also carries the coverage assertions.

The panel-blocked form is built by thresholds and run with a depth that are read once per process: its cases run in one fresh
child process per knob set (three), this file run as a script: `python tests/test_structured_branches_gpu.py <knob set>`.

Measured on an MI355X, largest error / bound per group, device | oracle (the two flavours of a group agree to the digits shown
unless two figures are given); cases per (type, flavour):
  row patterns, plain product (56 cases)       f64 0.200 | 0.200      f32 0.499 | 0.499
  row patterns, fused product (125)            f64 0.393 | 0.393      f32 0.500 | 0.500
  row patterns, deferred tail (4)              f64 0.268 / 0.248 | 0.314      f32 0.480 | 0.480
  row patterns, Chebyshev step (54)            f64 0.157 | 0.199      f32 0.494 | 0.878 (the oracle's product is stored in T first)
  stencil (63, and one declined complex case per complex type)     f64 0.188 | 0.188      f32 0.500 | 0.500
  panel-blocked (6 per type and knob set)      f64 0.190 | 0.190      f32 0.499 | 0.499 in all three processes
1246 cases in all.  The 22 in-process tests take 3.4 s together, the three child processes 2.6 to 2.8 s each: 12 s inside a
GPU suite that takes 669 s with this file (657 s without it, the build of the extensions included)."""
import os
import subprocess
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
if __name__ == "__main__":
    ROOT = os.path.dirname(HERE)
    sys.path[:0] = [ROOT, os.path.join(ROOT, "oracle"), HERE]

from kernel_harness import Dev
import structured_branch_cases as B

pytestmark = pytest.mark.gpu

GROUPS = B.groups()
KNOB_SETS = list(B.PB_KNOBS)


@pytest.mark.parametrize("gid,cases", GROUPS, ids=[g for g, _ in GROUPS])
def test_device_against_longdouble_reference(built, gid, cases):
    rep = B.run_cases(Dev, cases)
    print(f"{gid}: {rep.summary()}")
    assert not rep.fails, f"{gid}: {rep.summary()}\n" + "\n".join(rep.fails[:20])


@pytest.mark.parametrize("knobs", KNOB_SETS)
def test_panel_blocked_in_a_fresh_process(built, knobs):
    """one child at a time, the knob set in its environment; the child asserts through hipk_csr_format / hipk_csr_panels that its
    matrices are held in the panel-blocked form as pb_plan restates it, runs them against the same references and bounds, and
    prints `<knob set>: ok`"""
    env = dict(os.environ, **B.PB_KNOBS[knobs]["env"])
    p = subprocess.run([sys.executable, os.path.abspath(__file__), knobs], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True,
                       env=env, timeout=120)
    print(p.stdout[-2000:])
    assert p.returncode == 0 and f"{knobs}: ok" in p.stdout, p.stdout[-4000:]


if __name__ == "__main__":
    assert len(sys.argv) == 2 and sys.argv[1] in KNOB_SETS
    knobs = sys.argv[1]
    assert all(os.environ.get(k) == v for k, v in B.PB_KNOBS[knobs]["env"].items())
    assert all(os.environ.get(k) is None for k in ("HIPK_PB_U", "HIPK_PB_TILE") if k not in B.PB_KNOBS[knobs]["env"])
    failed = False
    for gid, cases in B.groups(knobs=True):
        if not gid.startswith(f"{knobs}-"):
            continue
        rep = B.run_cases(Dev, cases)
        print(f"{gid}: {rep.summary()}")
        if rep.fails:
            print("\n".join(rep.fails[:20]))
            failed = True
    if failed:
        sys.exit(1)
    print(f"{knobs}: ok")
