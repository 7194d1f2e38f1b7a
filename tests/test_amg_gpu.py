"""The aggregation algebraic multigrid preconditioner in the eigensolvers on the MI355X: precond=("amg", ...) of eigsh /
Session.solve (primme_amd/api.py -> primme_amd_operator_set_amg, primme_amd_amg_precond).  The 2-D CSR Laplacian at two grid
sizes against its analytic spectrum and against the same solve without a preconditioner (fewer outer iterations at both sizes,
and a count that grows less from the small grid to the large one), LUNDA.mtx under GD+k and JDQMR, in float32 and in a block of
4, its block-diagonal tiling, -Laplacian + V with shift about the mean of V, each against the dense truth with
resNorm <= eps |A|; and the ValueError cases of the Python layer.

Outer iterations measured on the MI355X: see DESIGN.md section 4o."""
import numpy as np
import pytest

import amg_cases as AMG
from checkers import Operator, Session, eigsh
from primme_amd import problems

pytestmark = pytest.mark.gpu
_counts = {}


def _lap2d(dims):
    """(plain, preconditioned) solves of the 2-D CSR Laplacian: computed once per grid and shared"""
    if dims not in _counts:
        rp, ci, va, n = problems.laplacian_csr(dims)
        op = Operator(n, csr=(rp, ci, va))
        kw = dict(numEvals=6, method="GD_plusK", eps=1e-10, aNorm=8.0, v0=problems.start_vector(n))
        _counts[dims] = (eigsh(op, backend="hip", **kw), eigsh(op, backend="hip", precond=("amg",), **kw))
    return _counts[dims]


@pytest.mark.parametrize("dims", [(33, 35), (129, 131)])
def test_laplacian_2d(built, dims):
    plain, pre = _lap2d(dims)
    exact = problems.laplacian_eigenvalues(dims, 6)
    assert plain.ret == 0 and pre.ret == 0
    assert np.max(np.abs(pre.evals - exact)) <= 1e-9 * 8.0
    assert np.all(pre.resNorms <= 1e-10 * 8.0)
    its, itp = plain.stats["numOuterIterations"], pre.stats["numOuterIterations"]
    print(f"{dims}: outer iterations {its} without, {itp} with the algebraic multigrid preconditioner; {pre.precond_stats}")
    assert itp < its
    assert pre.precond_stats["applies"] == pre.stats["numPreconds"] > 0 and pre.precond_stats["levels"] >= 2


def test_iteration_growth_with_the_grid(built):
    (p33, m33), (p129, m129) = _lap2d((33, 35)), _lap2d((129, 131))
    plain = p129.stats["numOuterIterations"] / p33.stats["numOuterIterations"]
    pre = m129.stats["numOuterIterations"] / m33.stats["numOuterIterations"]
    print(f"growth of the outer iterations from (33, 35) to (129, 131): {plain:.2f}x without, {pre:.2f}x with the preconditioner")
    assert pre < plain


_truth = {}


def _dense_truth(name, csr, k):
    if name not in _truth:
        rp, ci, va = csr
        _truth[name] = np.linalg.eigvalsh(AMG.dense(len(rp) - 1, rp, ci, va))
    return _truth[name][:k], float(np.abs(_truth[name]).max())


def _solve(name, csr, precond, k=4, dtype=np.float64, eps=1e-10, **kw):
    """one solve against the dense truth: resNorm <= eps |A|, and eigenvalues within 2 eps |A|: a Ritz value lies within its
    true residual norm of an eigenvalue, and the true residual is the reported one (<= eps |A|) plus the rounding of one
    product, of the order of the machine epsilon times |A|, below eps |A| for the eps used here; returns the result"""
    rp, ci, va = csr
    n = len(rp) - 1
    exact, aN = _dense_truth(name, csr, k)
    kw = dict(dict(numEvals=k, method="GD_plusK", eps=eps, aNorm=aN, v0=problems.start_vector(n)), **kw)
    r = eigsh(Operator(n, csr=csr), backend="hip", dtype=dtype, precond=precond, **kw)
    assert r.ret == 0, r.ret
    err = float(np.max(np.abs(np.sort(np.asarray(r.evals, dtype=np.float64)) - exact)))
    print(f"{name} {precond} {np.dtype(dtype).name} {kw['method']} block {kw.get('maxBlockSize', 1)}: outer iterations "
          f"{r.stats['numOuterIterations']}, matvecs {r.stats['numMatvecs']}, |evals - truth| = {err:.2e} (|A| = {aN:.3e}), {r.precond_stats}")
    assert err <= 2 * eps * aN
    assert np.all(np.asarray(r.resNorms, dtype=np.float64) <= eps * aN)
    return r


def test_lunda_gdk_jacobi_against_amg(built):
    """recorded, not asserted: the counts of Jacobi and of the algebraic multigrid preconditioner on LUNDA.mtx"""
    jac = _solve("lunda", AMG.lunda(), "jacobi")
    amg = _solve("lunda", AMG.lunda(), ("amg",))
    assert amg.precond_stats["applies"] == amg.stats["numPreconds"] > 0 and amg.precond_stats["levels"] == 1
    print(f"LUNDA GD+k: outer iterations {jac.stats['numOuterIterations']} with Jacobi, {amg.stats['numOuterIterations']} with AMG")


def test_lunda_jdqmr(built):
    _solve("lunda", AMG.lunda(), "jacobi", method="JDQMR")
    _solve("lunda", AMG.lunda(), ("amg",), method="JDQMR")


def test_lunda_float32(built):
    _solve("lunda", AMG.lunda(), ("amg",), dtype=np.float32, eps=2e-6)


def test_lunda_block_of_4(built):
    v0 = np.stack([problems.start_vector(147, j=j) for j in range(4)], axis=1)
    _solve("lunda", AMG.lunda(), ("amg", 2, 16), maxBlockSize=4, v0=v0)


def test_lunda_tiled(built):
    """four tiles (588 rows): two levels, the hierarchy of bench.py's configs[2] in small"""
    jac = _solve("lunda_x4", AMG.lunda_tiled(4), "jacobi", method="JDQMR")
    amg = _solve("lunda_x4", AMG.lunda_tiled(4), ("amg",), method="JDQMR")
    assert amg.precond_stats["levels"] == 2
    print(f"LUNDA x 4 JDQMR: outer iterations {jac.stats['numOuterIterations']} with Jacobi, {amg.stats['numOuterIterations']} with AMG")


def test_schrodinger(built):
    """-Laplacian + V; K^-1 for the matrix + shift, shift about the mean of V (the issue's setting)"""
    dims = (33, 35)
    i = np.arange(33 * 35)
    V = 0.5 + 0.4 * np.sin(0.37 * (i % 33)) * np.cos(0.23 * (i // 33))
    csr = problems.schrodinger_csr(dims, V)[:3]
    plain = _solve("schrodinger", csr, None)
    pre = _solve("schrodinger", csr, ("amg", 2, 16, 0.08, 1.0, float(V.mean())))
    assert pre.stats["numOuterIterations"] < plain.stats["numOuterIterations"]


def test_python_layer_refuses(built):
    rp, ci, va, n = problems.laplacian_csr((6, 7))
    op = Operator(n, csr=(rp, ci, va))
    cb = object()
    with pytest.raises(ValueError, match="user_precond"):
        eigsh(op, backend="hip", precond=("amg",), user_precond=cb)
    with pytest.raises(ValueError, match="real"):
        eigsh(op, backend="hip", dtype=np.complex128, precond=("amg",))
    with pytest.raises(ValueError, match="back end"):
        eigsh(op, backend="hostcheck", precond=("amg",))
    with pytest.raises(ValueError, match="stencil"):
        eigsh(Operator(42, stencil=(6, 7, 1)), backend="hip", precond=("amg",))
    with pytest.raises(ValueError, match="smooth_steps"):
        eigsh(op, backend="hip", precond=("amg", 2, 16, 0.08, 1.0, 0.0, 1))
    for bad in (("amg", 0), ("amg", 2, 0), ("amg", 2, 16, 1.0), ("amg", 2, 16, -0.1), ("amg", 2, 16, 0.08, 0.5), ("amg", 2, 16, 0.08, 2.0),
                ("amg", 2, 16, 0.08, 1.0, -1.0)):
        with pytest.raises(ValueError):
            eigsh(op, backend="hip", precond=bad)
    vb = va.copy()
    vb[ci == np.repeat(np.arange(n), np.diff(rp))] = -4.0
    with pytest.raises(ValueError, match="positive diagonal"):
        eigsh(Operator(n, csr=(rp, ci, vb)), backend="hip", precond=("amg",))
    s = Session(op, backend="hip")
    try:
        s.comm = object()                           # a row-partitioned session: refused before anything looks at the handle
        with pytest.raises(ValueError, match="single-rank"):
            s.solve(numEvals=1, precond=("amg",))
    finally:
        s.comm = None
        s.close()
