"""The numpy restatement of the device set-up of smoothed aggregation (tests/amg_hierarchy_cases.py) against the host plan
(primme_amd_amg_plan_create_smoothed through the CPU checker library), and the argument errors of primme_amd.AmgHierarchy and of
precond=("amg_hierarchy", ...), all without a GPU.

Per level of every matrix of amg_hierarchy_cases.matrices() and omega in {4/3, 0.5}: rowptr and colind of P, R and M_{l+1}
identical, the values of P and R the same bits (the checker library is built without contraction, -std=c99 on x86-64), the
coarse matrix within 32 eps sum|terms| per entry of the host's and exactly symmetric.  The restatement sums B = M P first and
then R B; the host sums the triple products in one loop: the largest fraction of the bound seen is printed (DESIGN.md 4q:
0.67 on the 1 x 1 coarse matrix of arrow_300 with omega 0.5, whose one entry has some 1500 terms; 0.40 on lunda_x4, 0.13 at most
on the grids)."""
import numpy as np
import pytest

import amg_hierarchy_cases as HC
import amg_smoothed_cases as SA
import checkers
import primme_amd
from primme_amd import problems

_mats = HC.matrices()
EXPECTED_ROWS = {"lap1d_1": [1], "lap1d_2": [2], "lap_6x7": [42], "lap_33x35": [1155, 206], "lap_65x67": [4355, 748, 120],
                 "diag_300": [300], "arrow_300": [300, 1], "lap_33x35_shift": [1155, 206]}


@pytest.mark.parametrize("omega", HC.OMEGAS)
@pytest.mark.parametrize("name", list(_mats))
def test_restatement_against_the_host_plan(built, name, omega):
    rp, ci, va, shift, theta = _mats[name]
    rc, lv, om = SA.c_plan(checkers.load_hostcheck(), rp, ci, va, shift=shift, theta=theta, omega=omega)
    assert rc == 0 and om == omega
    if name in EXPECTED_ROWS and (omega == HC.OMEGAS[0] or len(EXPECTED_ROWS[name]) < 3):      # omega changes M_1 and so level 2
        assert [v["n"] for v in lv] == EXPECTED_ROWS[name]
    else:
        assert len(lv) >= 2
    worst = 0.0
    for l in range(len(lv) - 1):
        v = lv[l]
        dinv, rho = HC.finish(v["rowptr"], v["colind"], v["values"])
        assert HC.same_bits(dinv, v["dinv"]) and rho == v["rho"]
        ref = HC.level(v["rowptr"], v["colind"], v["values"], v["dinv"], v["rho"], v["agg"], v["nc"], omega)
        worst = max(worst, HC.check_level(ref, ref, HC.host_level(v, lv[l + 1])))
    print(f"{name} omega {omega:.3f}: levels {[v['n'] for v in lv]}, largest |C - C_host| / (32 eps sum|terms|) = {worst:.4f}")


@pytest.mark.parametrize("name", list(HC.custom_cases()))
def test_restatement_on_the_custom_aggregates(name):
    """the cases the kernel tests add: the restatement is well formed there (sorted rows, symmetric C, P 1 = 1 - w D^-1 M 1)"""
    rp, ci, va, agg = HC.custom_cases()[name]
    n, nc = len(rp) - 1, int(agg.max()) + 1
    dinv, rho = HC.finish(rp, ci, va)
    ref = HC.level(rp, ci, va, dinv, rho, agg, nc, 4.0 / 3.0)
    prp, pci, pva = ref["P"]
    for i in range(n):
        assert np.all(np.diff(pci[prp[i]:prp[i + 1]]) > 0)
    rowsum = np.add.reduceat(va, rp[:-1])
    psum = np.add.reduceat(pva, prp[:-1])
    assert np.abs(psum - (1.0 - (4.0 / 3.0 / rho) * dinv * rowsum)).max() <= 1e-13
    assert HC.is_symmetric(*ref["C"]) and ref["C"][0][-1] == len(ref["C"][1])


def _op(dims=(6, 7)):
    rp, ci, va, _ = problems.laplacian_csr(dims)
    return primme_amd.Operator(len(rp) - 1, csr=(rp, ci, va))


def test_hierarchy_argument_errors():
    op = _op()
    with pytest.raises(ValueError, match="plain aggregation has setup='host'"):
        primme_amd.AmgHierarchy(op, smoothed=False, setup="device")
    with pytest.raises(ValueError, match="'host' or 'device'"):
        primme_amd.AmgHierarchy(op, setup="gpu")
    for kw in (dict(theta=1.0), dict(theta=-0.1), dict(omega=0.0), dict(omega=2.0), dict(shift=-1.0)):
        with pytest.raises(ValueError, match="needs 0 <= theta"):
            primme_amd.AmgHierarchy(op, **kw)
    with pytest.raises(ValueError, match="CSR arrays"):
        primme_amd.AmgHierarchy(primme_amd.Operator(42, stencil=(6, 7, 1)))
    H = primme_amd.AmgHierarchy(op)                                   # an Operator: built by the first solve
    assert not H.closed and (H.n, H.matrix_nnz) == (42, int(op.csr[0][-1]))
    with pytest.raises(ValueError, match="not built yet"):
        H.levels
    H.close()
    assert H.closed
    with pytest.raises(ValueError, match="closed"):
        H.plan()


def test_solve_argument_errors():
    """raised by Session.solve before any library call: a session over the CPU checker serves"""
    op = _op()
    s = primme_amd.Session(op, backend=checkers.HostcheckBackend())
    H = primme_amd.AmgHierarchy(op)
    for bad in (("amg_hierarchy",), ("amg_hierarchy", H, 2, 16, 1.0, 0.0)):
        with pytest.raises(ValueError, match=r"precond: \('amg_hierarchy', H"):
            s.solve(precond=bad)
    with pytest.raises(ValueError, match="is an AmgHierarchy"):
        s.solve(precond=("amg_hierarchy", 3))
    with pytest.raises(ValueError, match="over must be 1"):
        s.solve(precond=("amg_hierarchy", H, 2, 16, 1.5))
    for bad in (("amg_hierarchy", H, 0), ("amg_hierarchy", H, 2, 0), ("amg_hierarchy", primme_amd.AmgHierarchy(op, smoothed=False, setup="host"), 2, 16, 2.0)):
        with pytest.raises(ValueError, match="steps >= 1 and 1 <= over < 2"):
            s.solve(precond=bad)
    other = primme_amd.AmgHierarchy(_op((6, 8)))
    with pytest.raises(ValueError, match="48 rows"):
        s.solve(precond=("amg_hierarchy", other))
    with pytest.raises(ValueError, match="no such operator"):          # everything in order, but this back end has no device
        s.solve(precond=("amg_hierarchy", H))
    H.close()
    with pytest.raises(ValueError, match="H is closed"):
        s.solve(precond=("amg_hierarchy", H))
    s.close()
