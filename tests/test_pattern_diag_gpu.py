"""The diagonal-split flavour of the row-pattern form (csrc/hipk_sparse_pat.hip, HIPK_CSR_DIAG_PATTERNS of hipk_csr_create_opts):
stencil / lattice operators with a diagonal that differs from row to row keep one byte per row and stream the diagonal.

  products   y bit for bit the row-tile kernel's (same handle, hipk_set_spmv_format(0)), plain and fused, NaN-filled outputs;
             shapes of tests/test_kernels_gpu.py::test_csr_row_pattern_form with a random diagonal (full chunks only with a last
             pair that references the last column, a ragged last chunk with an odd row count, the width-8 lattice in two trips,
             a row slab with halo rows) and a lattice with diagonal-free rows whose pairs straddle a change of pattern
  flag off   the same matrix without the flag stays on the row tiles
  Chebyshev  hipk_csr_cheb_step in this form against the longdouble bound of tests/test_cheb_kernels_gpu.py and, in double, bit
             for bit against hipk_csr_matvec + hipk_cheb_update
  solves     -Laplacian + harmonic potential on 60 x 61 with Jacobi and Chebyshev preconditioning, with and without the flag
  C example  examples/ex_eigs_dhip_potential against numpy's spectrum of the same matrix"""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from kernel_harness import Dev, NPDT
from primme_amd import _ffi as F
from primme_amd import problems
from primme_amd.api import Operator, eigsh
from test_kernels_gpu import _lattice8_csr
from test_cheb_kernels_gpu import _Panel, _coef, _step_reference, _u, L
import test_solver_gpu as TS

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DTYPES = [F.HIPK_F64, F.HIPK_F32]
# the smallest relative band tests/test_solver_gpu.py applies to a count of a fixture whose history is not reproduced exactly
BAND = min(list(TS.LOOSE.values()) + list(TS.LOOSE_MATVECS.values()))


def _add_diagonal(rp, ci, va, row0, d):
    """va with d[i] ADDED to the diagonal entry of local row i (rows that store one)"""
    rows = np.repeat(np.arange(len(rp) - 1), np.diff(rp))
    va = np.array(va, dtype=np.float64)
    sel = ci == rows + row0
    va[sel] += d[rows[sel]]
    return va


def _lattice_holes(n, rng):
    """second-neighbour 1-D lattice, random diagonal, NO stored diagonal in every third row: with pairs of consecutive rows per lane
    the pattern changes inside two pairs out of three"""
    rows, cols, vals = [], [], []
    for i in range(n):
        for d, v in ((-2, 0.25), (-1, -1.0), (0, None), (1, -1.0), (2, 0.25)):
            if d == 0 and i % 3 == 0: continue
            if 0 <= i + d < n:
                rows.append(i); cols.append(i + d); vals.append(2.0 + rng.standard_normal() if v is None else v)
    rp = np.zeros(n + 1, dtype=np.int64); np.add.at(rp, np.array(rows) + 1, 1)
    return np.cumsum(rp).astype(np.int32), np.array(cols, dtype=np.int32), np.array(vals)


def _case(name):
    """-> rp, ci, va (double), n, row0, number of patterns expected (or None)"""
    rng = np.random.default_rng(17)
    row0, want = 0, None
    if name == "lap1d_full_chunks": rp, ci, va, n = problems.laplacian_csr((8192,)); want = 3
    elif name == "lap2d_full_chunks": rp, ci, va, n = problems.laplacian_csr((33, 512)); want = 9
    elif name == "lap2d_ragged": rp, ci, va, n = problems.laplacian_csr((37, 41)); want = 9
    elif name == "lattice8": n = 6001; rp, ci, va = _lattice8_csr(n)
    elif name == "lap3d_slab":
        dims = (23, 19, 17); n = int(np.prod(dims)); row0 = 2000
        rp, ci, va, _ = problems.laplacian_csr(dims, row0=row0, nrows=3003)
    elif name == "lattice_holes":
        n = 4099; rp, ci, va = _lattice_holes(n, rng)
        return rp, ci, va, n, 0, None
    else: raise ValueError(name)
    nloc = len(rp) - 1
    va = _add_diagonal(rp, ci, va, row0, rng.standard_normal(nloc) * 1.5)      # random, non-constant
    return rp, ci, va, n, row0, want


def _create(side, dt, rp, ci, va, n, row0, flags):
    A = C.c_void_p()
    vv = np.ascontiguousarray(va, dtype=NPDT[dt])
    assert side.lib.hipk_csr_create_opts(side.ctx, dt, len(rp) - 1, n, row0, rp.ctypes.data_as(C.c_void_p), ci.ctypes.data_as(C.c_void_p),
                                         vv.ctypes.data_as(C.c_void_p), flags, C.byref(A)) == 0
    return A


CASES = ["lap1d_full_chunks", "lap2d_full_chunks", "lap2d_ragged", "lattice8", "lap3d_slab", "lattice_holes"]


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("case", CASES)
def test_products_bit_for_bit(built, dt, case):
    npdt = NPDT[dt]
    rp, ci, va, n, row0, want = _case(case)
    nloc = len(rp) - 1
    rng = np.random.default_rng(23)
    side = Dev()
    lib = side.lib
    old = lib.hipk_set_spmv_format(1)
    try:
        # flag off: the diagonal makes every row its own pattern, the matrix stays on the row tiles
        A0 = _create(side, dt, rp, ci, va, n, row0, 0)
        assert lib.hipk_csr_format(A0) == 0 and lib.hipk_csr_pattern_diag(A0) == 0 and lib.hipk_csr_npatterns(A0) == 0
        lib.hipk_csr_destroy(A0)
        A = _create(side, dt, rp, ci, va, n, row0, F.HIPK_CSR_DIAG_PATTERNS)
        assert lib.hipk_csr_format(A) == 2 and lib.hipk_csr_pattern_diag(A) == 1
        if want: assert lib.hipk_csr_npatterns(A) == want
        es = np.dtype(npdt).itemsize
        assert lib.hipk_csr_product_bytes(A, 0) == nloc * (1 + 3 * es)
        assert lib.hipk_csr_product_bytes(A, 1) == nloc * (1 + 4 * es)
        Xg = rng.standard_normal(n) * 2.0
        lo, hi = int(lib.hipk_csr_halo_lo(A)), int(lib.hipk_csr_halo_hi(A))
        assert (lo > 0 and hi > 0) == (case == "lap3d_slab")
        x = side.arr(Xg[row0:row0 + nloc].astype(npdt))
        xlo = side.arr(Xg[row0 - lo:row0].astype(npdt) if lo else np.zeros(1, npdt))
        xhi = side.arr(Xg[row0 + nloc:row0 + nloc + hi].astype(npdt) if hi else np.zeros(1, npdt))
        assert lib.hipk_csr_set_halo_ld(A, side.ptr(xlo), max(lo, 1), side.ptr(xhi), max(hi, 1)) == 0
        nn = side.arr(np.array([float(np.sum(Xg ** 2))]))
        got = {}
        for fmt in (1, 0):
            lib.hipk_set_spmv_format(fmt)
            assert lib.hipk_csr_format(A) == (2 if fmt else 0) and lib.hipk_csr_pattern_diag(A) == fmt
            y = side.arr(np.full(nloc, np.nan, npdt)); yf = side.arr(np.full(nloc, np.nan, npdt)); xo = side.arr(np.full(nloc, np.nan, npdt))
            dot = side.arr(np.zeros(1))
            assert lib.hipk_csr_matvec(A, None, side.ptr(x), nloc, side.ptr(y), nloc, 1) == 0
            assert lib.hipk_csr_matvec_scaled(A, side.ctx, side.ptr(x), side.ptr(nn), side.ptr(xo), side.ptr(yf), side.ptr(dot)) == 0
            got[fmt] = [side.get(t) for t in (y, yf, xo, dot)]
        lib.hipk_csr_destroy(A)
    finally:
        lib.hipk_set_spmv_format(old)
        side.close()
    for t in range(3):
        assert not np.any(np.isnan(got[1][t])) and np.array_equal(got[1][t], got[0][t]), (case, t)     # bit for bit
    tol = 1e-12 if dt == F.HIPK_F64 else 2e-4                                                          # those of test_csr_row_pattern_form
    assert abs(got[1][3][0] - got[0][3][0]) <= tol * np.sqrt(nloc) * (1 + abs(got[0][3][0]))
    xin = Xg.astype(npdt).astype(np.float64)
    ref = np.zeros(nloc)
    np.add.at(ref, np.repeat(np.arange(nloc), np.diff(rp)), va.astype(npdt).astype(np.float64) * xin[ci])
    assert np.max(np.abs(got[1][0] - ref)) <= tol * 10 * (1 + np.abs(ref).max())
    a = 1.0 / np.sqrt(float(np.sum(Xg ** 2)))
    assert np.max(np.abs(got[1][1] - a * ref)) <= tol * 10 * (1 + np.abs(a * ref).max())
    assert abs(got[1][3][0] - a * a * float(xin[row0:row0 + nloc] @ ref)) <= tol * 50 * np.sqrt(nloc) * (1 + abs(got[1][3][0]))


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("case", ["lap2d_full_chunks", "lattice8"])
def test_fused_chebyshev_step(built, dt, case):
    """hipk_csr_cheb_step in the diagonal-split form, 1 and 3 columns, with and without Yprev: every element within
    B_i = u_T |ref_i| + 2 (len_i + 4) 2^-53 S_i of the longdouble reference (tests/test_cheb_kernels_gpu.py), and in double the
    bits of hipk_csr_matvec followed by hipk_cheb_update"""
    npdt = NPDT[dt]
    rp, ci, va, n, row0, _ = _case(case)
    rng = np.random.default_rng(n + 7)
    Yk, Yp, X = (rng.standard_normal((n, 8)).astype(npdt) for _ in range(3))
    cf, coefs = _coef()
    refs = _step_reference(rp, ci, np.asarray(va).astype(npdt), Yk, Yp, X, coefs)
    lens = np.diff(rp).astype(L)[:, None]
    ldx, ldk, ldp, ldo, ldw, ldq = n + 3, n + 5, n + 8, n + 13, n + 17, n + 21
    side = Dev()
    lib = side.lib
    old = lib.hipk_set_spmv_format(1)
    try:
        A = _create(side, dt, rp, ci, va, n, 0, F.HIPK_CSR_DIAG_PATTERNS)
        assert lib.hipk_csr_format(A) == 2 and lib.hipk_csr_pattern_diag(A) == 1
        st = lib.hipk_ctx_stream(side.ctx)
        es = np.dtype(npdt).itemsize
        for nx in (1, 3):
            px, pk = _Panel(side, X[:, :nx], ldx), _Panel(side, Yk[:, :nx], ldk)
            for prev in (True, False):
                pp = _Panel(side, Yp[:, :nx], ldp) if prev else None
                po = _Panel(side, None, ldo, shape=(n, nx, npdt))
                assert lib.hipk_csr_cheb_step(A, None, nx, C.byref(cf), px.ptr, ldx, pk.ptr, ldk, pp.ptr if pp else None, ldp, po.ptr, ldo) == 0
                out, raw = po.read()
                tag = f"{case} nx={nx} prev={prev}"
                assert not np.any(np.isnan(out)), tag
                assert po.outside_unchanged(raw) and px.unchanged() and pk.unchanged() and (pp is None or pp.unchanged()), tag
                ref, S = refs[prev]
                ref, S = ref[:, :nx], S[:, :nx]
                B = _u(npdt) * np.abs(ref) + 2 * (lens + 4) * L(2.0) ** -53 * S
                err = np.abs(out.astype(L) - ref)
                print(f"{tag}: max err/B = {float(np.max(err / B)):.3f}")
                assert np.all(err <= B), tag
                if dt == F.HIPK_F64:
                    pw, pq = _Panel(side, None, ldw, shape=(n, nx, npdt)), _Panel(side, None, ldq, shape=(n, nx, npdt))
                    for c in range(nx):
                        assert lib.hipk_csr_matvec(A, None, C.c_void_p(pk.ptr.value + c * ldk * es), ldk, C.c_void_p(pw.ptr.value + c * ldw * es), ldw, 1) == 0
                    assert lib.hipk_cheb_update(st, dt, n, nx, C.byref(cf), px.ptr, ldx, pw.ptr, ldw, pk.ptr, ldk, pp.ptr if pp else None, ldp,
                                                pq.ptr, ldq) == 0
                    assert np.array_equal(pq.read()[0], out), tag
        lib.hipk_csr_destroy(A)
    finally:
        lib.hipk_set_spmv_format(old)
        side.close()


def _oscillator(dims, w):
    nx, ny = dims
    return lambda g: w * w * (((g % nx) - 0.5 * (nx - 1)) ** 2 + ((g // nx) - 0.5 * (ny - 1)) ** 2)


def _dense(rp, ci, va, n):
    M = np.zeros((n, n))
    M[np.repeat(np.arange(n), np.diff(rp)), ci] = va
    return M


@pytest.fixture(scope="module")
def oscillator_60x61():
    dims = (60, 61)
    rp, ci, va, n = problems.schrodinger_csr(dims, _oscillator(dims, 0.06))
    lam = np.linalg.eigvalsh(_dense(rp, ci, va, n))
    return rp, ci, va, n, lam


@pytest.mark.parametrize("precond", ["jacobi", "chebyshev"])
def test_solves(built, oscillator_60x61, precond):
    """3 smallest of -Laplacian + harmonic potential, GD+k, eps 1e-8, with the diagonal-split form and on the row tiles: both
    reach numpy's eigenvalues; the operation counts agree within the band of a history that is not reproduced bit for bit (the
    fused tail's t'At has another summation order)."""
    rp, ci, va, n, lam = oscillator_60x61
    eps, anorm = 1e-8, float(np.max(np.abs(lam)))
    pc = "jacobi" if precond == "jacobi" else ("chebyshev", 8, float(0.5 * (lam[2] + lam[3])), None)
    res = {}
    for flag in (True, False):
        op = Operator(n, csr=(rp, ci, va), diag_patterns=flag)
        r = eigsh(op, numEvals=3, method="GD_plusK", eps=eps, aNorm=anorm, v0=problems.start_vector(n), precond=pc)
        assert r.ret == 0 and r.initSize == 3
        assert np.max(np.abs(np.sort(r.evals) - lam[:3])) <= eps * anorm, (flag, r.evals, lam[:3])
        assert np.all(r.resNorms <= eps * anorm), (flag, r.resNorms)
        if precond == "chebyshev" and flag:
            assert r.precond_stats["fused_steps"] > 0, r.precond_stats
        res[flag] = r.stats["numMatvecs"]
    print(precond, "numMatvecs with / without the flag:", res[True], res[False])
    assert abs(res[True] - res[False]) <= BAND * max(res[True], res[False]), res


def test_session_reports_the_form(built, oscillator_60x61):
    """Operator(diag_patterns=True) reaches hipk_csr_create_opts: the Session's matrix handle is in the diagonal-split form"""
    from primme_amd.api import Session
    rp, ci, va, n, _ = oscillator_60x61
    for flag in (True, False):
        s = Session(Operator(n, csr=(rp, ci, va), diag_patterns=flag))
        try:
            A = dict((k, h) for k, h in s.handles)["csr"]
            assert s.lib.hipk_csr_pattern_diag(A) == int(flag) and s.lib.hipk_csr_format(A) == (2 if flag else 0)
        finally:
            s.close()


def test_c_example(built):
    """examples/ex_eigs_dhip_potential: builds, returns 0 and prints the six smallest eigenvalues of its 48 x 48 oscillator"""
    exe = os.path.join(ROOT, "examples", "ex_eigs_dhip_potential")
    if not os.path.exists(exe):
        subprocess.check_call(["make", "-C", os.path.join(ROOT, "examples")])
    out = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300)
    assert out.returncode == 0, out.stdout[-2000:]
    assert re.search(r"format 2, 9 row patterns, diagonal streamed: 1", out.stdout), out.stdout
    got = np.array([float(v) for v in re.findall(r"eval\[\d\] = (\S+)", out.stdout)])
    dims = (48, 48)
    rp, ci, va, n = problems.schrodinger_csr(dims, _oscillator(dims, 0.05))
    lam = np.linalg.eigvalsh(_dense(rp, ci, va, n))
    assert got.shape == (6,)
    assert np.max(np.abs(np.sort(got) - lam[:6])) <= 1e-9 * float(np.max(np.abs(lam))), (got, lam[:6])
