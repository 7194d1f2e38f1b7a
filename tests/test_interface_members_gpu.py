"""Members by name on the device: the C example that includes primme.h only, and members= of the Python drivers against the
same solves set up through the existing keyword arguments and tweak."""
import math
import os
import re
import subprocess

import numpy as np
import pytest

from primme_amd import problems

import checkers

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N = 100


def test_example_sets_members_by_name(built):
    exe = os.path.join(ROOT, "examples", "ex_eigs_members")
    if not os.path.exists(exe):
        subprocess.check_call(["make", "-C", os.path.join(ROOT, "examples")])
    out = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=120)
    assert out.returncode == 0, out.stdout[-2000:]
    # the listing the reference prints for the same settings (tests/golden/make_interface_golden.py)
    gold = open(os.path.join(ROOT, "tests", "golden", "display_ex_eigs_members.txt")).read()
    assert out.stdout.startswith(gold), out.stdout[:3000]
    rest = out.stdout[len(gold):]
    assert re.match(r"dprimme returned 0: 5 pairs, \d+ outer iterations, \d+ matvecs, \d+ restarts\n", rest), rest[:300]
    evals = [float(v) for v in re.findall(r"^Eval\[\d\] = (\S+)", rest, flags=re.M)]
    exact = [2.0 - 2.0 * math.cos(k * math.pi / (N + 1)) for k in range(1, 6)]
    assert len(evals) == 5
    # the example's eps = 1e-9 times |A| (the 1-D Laplacian's norm is below 4)
    assert max(abs(a - b) for a, b in zip(evals, exact)) <= 1e-9 * 4.0


@pytest.fixture(scope="module")
def lap():
    rp, ci, va, n = problems.laplacian_csr((N,))
    return checkers.Operator(n, csr=(rp, ci, va)), problems.start_vector(n)


def same(a, b):
    assert a.ret == b.ret == 0
    assert np.array_equal(a.evals, b.evals) and np.array_equal(a.resNorms, b.resNorms)
    assert a.stats["numOuterIterations"] == b.stats["numOuterIterations"] and a.stats["numMatvecs"] == b.stats["numMatvecs"]
    assert a.params == b.params


def test_members_equal_keywords_and_tweak(built, lap):
    op, v0 = lap
    kw = dict(numEvals=3, eps=1e-9, aNorm=4.0, v0=v0, method="JDQMR")

    def no_inner(p):
        p.correctionParams.maxInnerIterations = 0
    a = checkers.eigsh(op, members={"maxBasisSize": 12, "minRestartSize": 4, "correctionParams.maxInnerIterations": 0}, **kw)
    b = checkers.eigsh(op, maxBasisSize=12, minRestartSize=4, tweak=no_inner, **kw)
    same(a, b)
    assert a.params["maxBasisSize"] == 12 and a.params["minRestartSize"] == 4
    # ... and the members did something: JDQMR with its inner iterations takes another path
    c = checkers.eigsh(op, maxBasisSize=12, minRestartSize=4, **kw)
    assert c.ret == 0 and c.stats["numMatvecs"] != a.stats["numMatvecs"]


def test_enum_member_by_constant_name(built, lap):
    op, v0 = lap
    kw = dict(numEvals=2, eps=1e-9, aNorm=4.0, v0=v0, target="closest_abs", targetShifts=[1.0], maxBasisSize=20)
    a = checkers.eigsh(op, members={"projectionParams.projection": "primme_proj_refined"}, **kw)
    b = checkers.eigsh(op, projection="refined", **kw)
    same(a, b)
    assert np.max(np.abs(a.evals - 1.0)) < 0.1


def test_unknown_member_or_constant_is_a_value_error(built, lap):
    op, v0 = lap
    with pytest.raises(ValueError, match="noSuchMember"):
        checkers.eigsh(op, numEvals=1, v0=v0, members={"noSuchMember": 1})
    with pytest.raises(ValueError, match="primme_proj_nonsense"):
        checkers.eigsh(op, numEvals=1, v0=v0, members={"projectionParams.projection": "primme_proj_nonsense"})


def test_svds_members_reach_the_eigensolver_block(built):
    m, n = 120, N
    rng = np.random.default_rng(5)
    dense = np.where(rng.random((m, n)) < 0.08, rng.standard_normal((m, n)), 0.0) + np.eye(m, n) * np.linspace(1.0, 3.0, n)
    rows, cols = np.nonzero(dense)
    rp = np.concatenate(([0], np.cumsum(np.bincount(rows, minlength=m)))).astype(np.int32)
    csr = (rp, cols.astype(np.int32), dense[rows, cols])
    # a fixed first-stage method: the default, PRIMME_DYNAMIC, chooses between GD+k and JDQMR by the times it measures, and
    # two runs of one and the same parameter block then differ in their iteration counts and last bits
    kw = dict(numSvals=3, eps=1e-9, iseed=[1, 2, 3, 4], methodStage1="GD_plusK")

    def basis(ps):
        ps.primme.maxBasisSize = 12
    a = checkers.svds(m, n, csr, members={"primme.maxBasisSize": 12}, **kw)
    b = checkers.svds(m, n, csr, tweak=basis, **kw)
    assert a.ret == b.ret == 0 and a.params["maxBasisSize"] == b.params["maxBasisSize"] == 12
    assert np.array_equal(a.svals, b.svals) and np.array_equal(a.resNorms, b.resNorms)
    assert a.eig_stats["numOuterIterations"] == b.eig_stats["numOuterIterations"]
    exact = np.linalg.svd(dense, compute_uv=False)[:3]
    assert np.max(np.abs(np.sort(a.svals)[::-1] - exact)) <= 1e-8 * exact[0]
    with pytest.raises(ValueError, match="noSuchMember"):
        checkers.svds(m, n, csr, members={"primme.noSuchMember": 1}, **kw)
