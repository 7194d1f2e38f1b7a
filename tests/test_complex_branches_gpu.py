"""Every dispatch branch of the complex panel, Ritz and column kernels (csrc/hipk_complex.hip) and of hipk_copy_cols at small
sizes (-m gpu): the cases of tests/complex_branch_cases.py on the device against the clongdouble references written from the
header's contract, with the derived bounds and the guard / padding comparison of every operand.  One test per (table, type,
flavour); its cases run on one context.  The same cases run on the plain-C oracle in tests/test_complex_branches_host.py,
which also asserts that the tables cover every instantiation.

Run as a script (`python tests/test_complex_branches_gpu.py nosplit`) this file is the child process of
test_ritz_update_one_lane_forms_only: HIPK_Z_NO_SPLIT is read once per process."""
import os
import subprocess
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
if __name__ == "__main__":
    ROOT = os.path.dirname(HERE)
    sys.path[:0] = [ROOT, os.path.join(ROOT, "oracle"), HERE]

from kernel_harness import Dev
import complex_branch_cases as Z

pytestmark = pytest.mark.gpu

GROUPS = Z.groups([tb for tb in Z.TABLES if tb != "dots_mfma"])
MFMA_GROUPS = Z.groups(["dots_mfma"])


@pytest.mark.parametrize("gid,cases", GROUPS, ids=[g for g, _ in GROUPS])
def test_device_against_longdouble_reference(built, gid, cases):
    rep = Z.run_cases(Dev, cases)
    print(f"{gid}: {rep.summary()}")
    assert not rep.fails, f"{gid}: {rep.summary()}\n" + "\n".join(rep.fails[:20])


@pytest.mark.parametrize("gid,cases", MFMA_GROUPS, ids=[g for g, _ in MFMA_GROUPS])
def test_dots_on_the_matrix_cores(built, gid, cases):
    """zdots_mfma_kernel is opt-in: the runner switches it on with hipk_set_zdots_mfma(1) around each call (and restores the
    previous value in a finally), runs the same inputs on the vector units and compares both with the reference and with
    each other.  The case that enters the grid-halving loop needs enough workgroups for this device's CU count."""
    import torch
    num_cu = torch.cuda.get_device_properties(0).multi_processor_count
    mbpc = int(os.environ.get("HIPK_ZMFMA_BPC") or 2)
    run = []
    for c in cases:
        if c.get("halving") and not Z.mfma_halves(c, num_cu, max(mbpc, 1)):
            print(f"{Z.case_id(c)}: left out, {num_cu} CUs take its grid without halving (the cell ('halving', ...) is not covered on this device)")
            continue
        run.append(c)
    rep = Z.run_cases(Dev, run)
    print(f"{gid}: {rep.summary()}")
    assert not rep.fails, f"{gid}: {rep.summary()}\n" + "\n".join(rep.fails[:20])
    from primme_amd import _ffi as F
    lib = F.load_product()                 # the switch is process-wide: it must have come back as it was
    old = lib.hipk_set_zdots_mfma(0)
    lib.hipk_set_zdots_mfma(old)
    assert old == (1 if os.environ.get("HIPK_ZMFMA", "0") not in ("", "0") and "HIPK_NO_MFMA" not in os.environ else 0)


def test_ritz_update_one_lane_forms_only(built):
    """HIPK_Z_NO_SPLIT=1 keeps hipk_ritz_update on the one-lane-per-row kernels (every list of more than 16 + 16 jobs then
    takes the chunked path), and the knob is read once per process: one fresh child runs the ritz_update table with it"""
    env = dict(os.environ, HIPK_Z_NO_SPLIT="1")
    p = subprocess.run([sys.executable, os.path.abspath(__file__), "nosplit"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True,
                       env=env, timeout=180)
    print(p.stdout[-2000:])
    assert p.returncode == 0 and "ritz_update (one lane per row): ok" in p.stdout, p.stdout[-4000:]


if __name__ == "__main__":
    assert sys.argv[1:] == ["nosplit"] and os.environ.get("HIPK_Z_NO_SPLIT")
    cases = Z.CASES["ritz_update"]
    assert all(x[0] == "zritz_kernel" for c in cases for x in Z.branch_of(c, nosplit=True))
    have, want, _ = Z.coverage("ritz_update", nosplit=True)
    assert not want - have
    rep = Z.run_cases(Dev, cases)
    print(f"ritz_update (one lane per row): {rep.summary()}")
    if rep.fails:
        print("\n".join(rep.fails[:20]))
        sys.exit(1)
    print("ritz_update (one lane per row): ok")
