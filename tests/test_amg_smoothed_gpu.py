"""Smoothed aggregation in the eigensolvers on the MI355X: precond=("amg_smoothed", ...) of eigsh / Session.solve
(primme_amd/api.py -> primme_amd_operator_set_amg_smoothed, primme_amd_amg_precond), with the set-up of tests/test_amg_gpu.py
(6 smallest, GD+k, eps 1e-10, aNorm 8).  The 2-D CSR Laplacian at 33 x 35 and 129 x 131 against its analytic spectrum and
against the same solve with ("amg",): fewer outer iterations at both sizes and a count that grows less from the small grid to
the large one.  The four tiles of LUNDA.mtx (588 rows, two levels) under JDQMR, in float32 and in a block of 4, and
-Laplacian + V with shift = mean V, each against the dense truth as test_amg_gpu.py::_solve compares; and the ValueError cases
of the Python layer.

Outer iterations measured on the MI355X: see DESIGN.md section 4p."""
import numpy as np
import pytest

import amg_cases as AMG
from checkers import Operator, Session, eigsh
from primme_amd import problems
from test_amg_gpu import _solve

pytestmark = pytest.mark.gpu
_counts = {}


def _lap2d(dims):
    """(plain aggregation, smoothed aggregation) solves of the 2-D CSR Laplacian: computed once per grid and shared"""
    if dims not in _counts:
        rp, ci, va, n = problems.laplacian_csr(dims)
        op = Operator(n, csr=(rp, ci, va))
        kw = dict(numEvals=6, method="GD_plusK", eps=1e-10, aNorm=8.0, v0=problems.start_vector(n))
        _counts[dims] = (eigsh(op, backend="hip", precond=("amg",), **kw), eigsh(op, backend="hip", precond=("amg_smoothed",), **kw))
    return _counts[dims]


@pytest.mark.parametrize("dims", [(33, 35), (129, 131)])
def test_laplacian_2d(built, dims):
    plain, sm = _lap2d(dims)
    exact = problems.laplacian_eigenvalues(dims, 6)
    assert plain.ret == 0 and sm.ret == 0
    assert np.max(np.abs(sm.evals - exact)) <= 1e-9 * 8.0
    assert np.all(sm.resNorms <= 1e-10 * 8.0)
    itp, its = plain.stats["numOuterIterations"], sm.stats["numOuterIterations"]
    print(f"{dims}: outer iterations {itp} with plain, {its} with smoothed aggregation; {plain.precond_stats} / {sm.precond_stats}")
    assert its < itp
    assert sm.precond_stats["applies"] == sm.stats["numPreconds"] > 0 and sm.precond_stats["levels"] >= 2
    assert sm.precond_stats.keys() == plain.precond_stats.keys()


def test_iteration_growth_with_the_grid(built):
    (p33, s33), (p129, s129) = _lap2d((33, 35)), _lap2d((129, 131))
    plain = p129.stats["numOuterIterations"] / p33.stats["numOuterIterations"]
    sm = s129.stats["numOuterIterations"] / s33.stats["numOuterIterations"]
    print(f"growth of the outer iterations from (33, 35) to (129, 131): {plain:.2f}x with plain, {sm:.2f}x with smoothed aggregation")
    assert sm < plain


def test_lunda_tiled_jdqmr(built):
    r = _solve("lunda_x4", AMG.lunda_tiled(4), ("amg_smoothed",), method="JDQMR")
    assert r.precond_stats["levels"] == 2 and r.precond_stats["applies"] == r.stats["numPreconds"] > 0


def test_lunda_tiled_float32(built):
    r = _solve("lunda_x4", AMG.lunda_tiled(4), ("amg_smoothed",), dtype=np.float32, eps=2e-6)
    assert r.precond_stats["levels"] == 2


def test_lunda_tiled_block_of_4(built):
    v0 = np.stack([problems.start_vector(588, j=j) for j in range(4)], axis=1)
    r = _solve("lunda_x4", AMG.lunda_tiled(4), ("amg_smoothed", 2, 16), maxBlockSize=4, v0=v0)
    assert r.precond_stats["levels"] == 2


def test_schrodinger(built):
    """-Laplacian + V; K^-1 for the matrix + shift, shift = the mean of V"""
    dims = (33, 35)
    i = np.arange(33 * 35)
    V = 0.5 + 0.4 * np.sin(0.37 * (i % 33)) * np.cos(0.23 * (i // 33))
    csr = problems.schrodinger_csr(dims, V)[:3]
    plain = _solve("schrodinger", csr, None)
    pre = _solve("schrodinger", csr, ("amg_smoothed", 2, 16, 0.08, 4.0 / 3.0, float(V.mean())))
    assert pre.stats["numOuterIterations"] < plain.stats["numOuterIterations"]


def test_python_layer_refuses(built):
    rp, ci, va, n = problems.laplacian_csr((6, 7))
    op = Operator(n, csr=(rp, ci, va))
    cb = object()
    S = "amg_smoothed"
    with pytest.raises(ValueError, match="user_precond"):
        eigsh(op, backend="hip", precond=(S,), user_precond=cb)
    with pytest.raises(ValueError, match="real"):
        eigsh(op, backend="hip", dtype=np.complex128, precond=(S,))
    with pytest.raises(ValueError, match="back end"):
        eigsh(op, backend="hostcheck", precond=(S,))
    with pytest.raises(ValueError, match="stencil"):
        eigsh(Operator(42, stencil=(6, 7, 1)), backend="hip", precond=(S,))
    with pytest.raises(ValueError, match="omega"):
        eigsh(op, backend="hip", precond=(S, 2, 16, 0.08, 4.0 / 3.0, 0.0, 1))
    for bad in ((S, 0), (S, 2, 0), (S, 2, 16, 1.0), (S, 2, 16, -0.1), (S, 2, 16, 0.08, 0.0), (S, 2, 16, 0.08, 2.0), (S, 2, 16, 0.08, -1.0),
                (S, 2, 16, 0.08, 1.0, -1.0)):
        with pytest.raises(ValueError):
            eigsh(op, backend="hip", precond=bad)
    vb = va.copy()
    vb[ci == np.repeat(np.arange(n), np.diff(rp))] = -4.0
    with pytest.raises(ValueError, match="positive diagonal"):
        eigsh(Operator(n, csr=(rp, ci, vb)), backend="hip", precond=(S,))
    s = Session(op, backend="hip")
    try:
        s.comm = object()                           # a row-partitioned session: refused before anything looks at the handle
        with pytest.raises(ValueError, match="single-rank"):
            s.solve(numEvals=1, precond=(S,))
    finally:
        s.comm = None
        s.close()
    # a good one on the same operator: over = 1 of ("amg",) is a valid omega here, and the seventh element of ("amg", ...) is still refused
    assert eigsh(op, backend="hip", precond=(S, 2, 16, 0.08, 1.0), numEvals=1, eps=1e-8, aNorm=8.0).ret == 0
    with pytest.raises(ValueError, match="smooth_steps"):
        eigsh(op, backend="hip", precond=("amg", 2, 16, 0.08, 1.0, 0.0, 1))
