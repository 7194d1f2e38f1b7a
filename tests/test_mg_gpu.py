"""The geometric multigrid preconditioner in the eigensolvers on the MI355X: precond=("multigrid", dims, ...) of eigsh /
Session.solve (primme_amd/api.py -> primme_amd_multigrid_precond).  The 2-D Laplacian at two grid sizes against its analytic
spectrum and against the same solve without a preconditioner (fewer outer iterations at both sizes, and a count that grows less
from the small grid to the large one), then one solve per solver feature the preconditioner has to live with: JDQMR (needs a
symmetric K), a 3-D grid, float32, a block of 4, the stencil operator form and -Laplacian + V in the diagonal-pattern form with
shift = mean(V); and the ValueError cases of the Python layer.

Outer iterations measured on the MI355X (6 smallest, GD+k, eps 1e-10, block size 1), without / with the preconditioner:
see DESIGN.md section 4n."""
import numpy as np
import pytest

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
        _counts[dims] = (eigsh(op, backend="hip", **kw), eigsh(op, backend="hip", precond=("multigrid", dims), **kw))
    return _counts[dims]


@pytest.mark.parametrize("dims", [(33, 35), (129, 131)])
def test_laplacian_2d(built, dims):
    plain, pre = _lap2d(dims)
    exact = problems.laplacian_eigenvalues(dims, 6)
    assert plain.ret == 0 and pre.ret == 0
    assert np.max(np.abs(pre.evals - exact)) <= 1e-9 * 8.0
    assert np.all(pre.resNorms <= 1e-10 * 8.0)
    its, itp = plain.stats["numOuterIterations"], pre.stats["numOuterIterations"]
    print(f"{dims}: outer iterations {its} without, {itp} with the multigrid preconditioner; {pre.precond_stats}")
    assert itp < its
    assert pre.precond_stats["applies"] == pre.stats["numPreconds"] > 0


def test_iteration_growth_with_the_grid(built):
    (p33, m33), (p129, m129) = _lap2d((33, 35)), _lap2d((129, 131))
    plain = p129.stats["numOuterIterations"] / p33.stats["numOuterIterations"]
    pre = m129.stats["numOuterIterations"] / m33.stats["numOuterIterations"]
    print(f"growth of the outer iterations from (33, 35) to (129, 131): {plain:.2f}x without, {pre:.2f}x with the preconditioner")
    assert pre < plain


def _pair(op, precond, aNorm, dtype=np.float64, **kw):
    """the same solve without and with the preconditioner: eigenvalues within 1e-8 aNorm, the preconditioner was applied"""
    kw = dict(dict(numEvals=4, method="GD_plusK", eps=1e-10, aNorm=aNorm, v0=problems.start_vector(op.n)), **kw)
    plain = eigsh(op, backend="hip", dtype=dtype, **kw)
    pre = eigsh(op, backend="hip", dtype=dtype, precond=precond, **kw)
    assert plain.ret == 0 and pre.ret == 0, (plain.ret, pre.ret)
    diff = float(np.max(np.abs(np.asarray(pre.evals, dtype=np.float64) - np.asarray(plain.evals, dtype=np.float64))))
    print(f"outer iterations {plain.stats['numOuterIterations']} -> {pre.stats['numOuterIterations']}, matvecs "
          f"{plain.stats['numMatvecs']} -> {pre.stats['numMatvecs']}, |evals - plain| = {diff:.2e} (allowed {1e-8 * aNorm:.1e}), {pre.precond_stats}")
    assert diff <= 1e-8 * aNorm
    assert pre.precond_stats["applies"] > 0 and pre.precond_stats["launches"] > 0
    return plain, pre


def test_jdqmr(built):
    rp, ci, va, n = problems.laplacian_csr((33, 35))
    _pair(Operator(n, csr=(rp, ci, va)), ("multigrid", (33, 35)), 8.0, method="JDQMR")


def test_3d(built):
    dims = (9, 10, 11)
    rp, ci, va, n = problems.laplacian_csr(dims)
    plain, pre = _pair(Operator(n, csr=(rp, ci, va)), ("multigrid", dims), 12.0)
    assert np.max(np.abs(pre.evals - problems.laplacian_eigenvalues(dims, 4))) <= 1e-9 * 12.0


def test_float32(built):
    rp, ci, va, n = problems.laplacian_csr((33, 35))
    _pair(Operator(n, csr=(rp, ci, va)), ("multigrid", (33, 35)), 8.0, dtype=np.float32, eps=2e-6)


def test_block_of_4(built):
    rp, ci, va, n = problems.laplacian_csr((33, 35))
    v0 = np.stack([problems.start_vector(n, j=j) for j in range(4)], axis=1)
    _pair(Operator(n, csr=(rp, ci, va)), ("multigrid", (33, 35), 2, 16), 8.0, maxBlockSize=4, v0=v0)


def test_stencil_operator(built):
    _pair(Operator(33 * 35, stencil=(33, 35, 1)), ("multigrid", (33, 35, 1)), 8.0)


def test_schrodinger_diag_patterns(built):
    """-Laplacian + V through the row-pattern form that streams the diagonal; K^-1 for -Laplacian + mean(V)"""
    dims = (33, 35)
    i = np.arange(33 * 35)
    V = 0.5 + 0.4 * np.sin(0.37 * (i % 33)) * np.cos(0.23 * (i // 33))
    rp, ci, va, n = problems.schrodinger_csr(dims, V)
    plain, pre = _pair(Operator(n, csr=(rp, ci, va), diag_patterns=True), ("multigrid", dims, 2, 16, 1.0, float(V.mean())), 8.0 + float(V.max()))
    assert pre.stats["numOuterIterations"] < plain.stats["numOuterIterations"]


def test_python_layer_refuses(built):
    rp, ci, va, n = problems.laplacian_csr((6, 7))
    op = Operator(n, csr=(rp, ci, va))
    cb = object()
    with pytest.raises(ValueError, match="user_precond"):
        eigsh(op, backend="hip", precond=("multigrid", (6, 7)), user_precond=cb)
    with pytest.raises(ValueError, match="real"):
        eigsh(op, backend="hip", dtype=np.complex128, precond=("multigrid", (6, 7)))
    with pytest.raises(ValueError, match="back end"):
        eigsh(op, backend="hostcheck", precond=("multigrid", (6, 7)))
    for bad in (("multigrid",), ("multigrid", (6, 7), 2, 16, 1.0, 0.0, 1)):
        with pytest.raises(ValueError, match="smooth_steps"):
            eigsh(op, backend="hip", precond=bad)
    for bad in (("multigrid", (6, 8)), ("multigrid", (6, 7), 0), ("multigrid", (6, 7), 2, 0), ("multigrid", (6, 7), 2, 16, 0.0),
                ("multigrid", (6, 7), 2, 16, 1.0, -1.0), ("multigrid", (6, 7, 1, 1))):
        with pytest.raises(ValueError):
            eigsh(op, backend="hip", precond=bad)
    s = Session(op, backend="hip")
    try:
        s.comm = object()                           # a row-partitioned session: refused before anything looks at the handle
        with pytest.raises(ValueError, match="single-rank"):
            s.solve(numEvals=1, precond=("multigrid", (6, 7)))
    finally:
        s.comm = None
        s.close()
