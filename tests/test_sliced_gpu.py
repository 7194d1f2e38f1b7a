"""The sliced-ELL form of a general CSR operator on the device (csrc/hipk_sparse_sell.hip; HIPK_CSR_SLICED of hipk_csr_create_opts,
Operator(sliced=True)).

  products   every shape of tests/test_sliced_host.py and a random band matrix with row lengths 0..21, 1 to 64 columns, ldx and ldy
             larger than m, y pre-filled with NaN.  Bound per entry against a longdouble product: a column is ONE fma chain over
             the row's len_i entries in double, so |y_i - ref_i| <= (len_i + 2) 2^-53 sum_j |a_ij| |x_j| (+ one rounding of the
             output in float).  The bound follows from the arithmetic; it is not measured.  Column c of a wide call equals the
             one-column call bit for bit; two runs agree bit for bit.
  padding    never contributes: NaN in x at columns no row references, and at the very columns the padding entries point at
  shifted    y = A x - shift x within the same bound, the shift term being one more entry of the chain
  fallback   too much padding, or an operator with halo: the flag is accepted, nothing is built, y is bit for bit that of a handle
             created without the flag
  switch     hipk_set_spmv_format(0) on the same handle: the row tiles, within twice the bound of the sliced result
  unrouted   hipk_csr_cheb_step, hipk_csr_matvec_scaled, hipk_csr_gershgorin: bit for bit those of an unflagged handle
  solves     LUNDA x 4, JDQMR block size 4 with Jacobi, and GD+k at block size 1, with and without sliced=True"""
import ctypes as C
import functools

import numpy as np
import pytest

from kernel_harness import Dev, NPDT
from primme_amd import _ffi as F
from primme_amd import problems
from primme_amd.api import Operator, Session, eigsh
from test_cheb_kernels_gpu import _coef
import checkers
import sliced_cases as SC
import test_solver_gpu as TS

pytestmark = pytest.mark.gpu
DTYPES = [F.HIPK_F64, F.HIPK_F32]
WIDTHS = [1, 3, 4, 8, 9, 64]
# the smallest relative band tests/test_solver_gpu.py grants a count whose history is not reproduced exactly
BAND = min(TS.LOOSE.values())
L = SC.L


def _create(side, dt, rp, ci, va, n, row0, flags):
    A = C.c_void_p()
    vv = np.ascontiguousarray(va, dtype=NPDT[dt])
    assert side.lib.hipk_csr_create_opts(side.ctx, dt, len(rp) - 1, n, row0, rp.ctypes.data_as(C.c_void_p), ci.ctypes.data_as(C.c_void_p),
                                         vv.ctypes.data_as(C.c_void_p), flags, C.byref(A)) == 0
    return A


class _Run:
    """X (m x k, device dtype) on the device with column stride ldx; products into NaN-filled buffers with column stride ldy"""

    def __init__(self, side, A, X, pad=(5, 11)):
        self.side, self.A, self.m, self.k = side, A, X.shape[0], X.shape[1]
        self.ldx, self.ldy = self.m + pad[0], self.m + pad[1]
        buf = np.full((self.k, self.ldx), np.nan, dtype=X.dtype)
        buf[:, :self.m] = X.T
        self.x = side.arr(buf.ravel())
        self.dtype = X.dtype

    def product(self, c0, nc, shift=None):
        """columns [c0, c0 + nc) -> m x nc; the rest of the output buffer must still hold its NaN"""
        side, lib = self.side, self.side.lib
        y = side.arr(np.full(nc * self.ldy, np.nan, dtype=self.dtype))
        if shift is None:
            assert lib.hipk_csr_matvec(self.A, None, side.ptr(self.x, c0 * self.ldx), self.ldx, side.ptr(y), self.ldy, nc) == 0
        else:
            sh = np.ascontiguousarray(shift, dtype=np.float64)
            assert lib.hipk_csr_matvec_shifted(self.A, None, side.ptr(self.x, c0 * self.ldx), self.ldx, side.ptr(y), self.ldy, nc,
                                               sh.ctypes.data_as(C.POINTER(C.c_double))) == 0
        raw = side.get(y).reshape(nc, self.ldy)
        assert np.all(np.isnan(raw[:, self.m:])), "rows of y beyond m were written"
        return raw[:, :self.m].T.copy()


@functools.lru_cache(maxsize=None)
def _reference(name, dt, k):
    """shared, read-only: values and X as the device holds them, longdouble product, |A||X|, bound"""
    rp, ci, va = SC.matrix(name)
    npdt = NPDT[dt]
    m = len(rp) - 1
    X = (np.random.default_rng(31 + m).standard_normal((m, k)) * 2.0).astype(npdt)
    vt = va.astype(npdt)
    ref, S = SC.product_reference(rp, ci, vt, X)
    out = (X, vt, ref, S, SC.product_bound(rp, ref, S, npdt))
    for a in out: a.setflags(write=False)
    return out


def _within(y, ref, B, tag):
    assert not np.any(np.isnan(y)), tag
    err = np.abs(y.astype(L) - ref)
    with np.errstate(divide="ignore", invalid="ignore"):
        worst = float(np.nanmax(np.where(B > 0, err / B, np.where(err > 0, np.inf, 0.0))))
    print(f"{tag}: max err / bound = {worst:.3f}")
    assert np.all(err <= B), tag


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("name", SC.SHAPES + ["random_band"])
def test_products(built, name, dt):
    rp, ci, va = SC.matrix(name)
    m = len(rp) - 1
    X, vt, ref, S, B = _reference(name, dt, 64)
    side = Dev()
    lib = side.lib
    old = lib.hipk_set_spmv_format(1)
    try:
        A = _create(side, dt, rp, ci, va, m, 0, F.HIPK_CSR_SLICED)
        assert lib.hipk_csr_sliced(A) == 1 and lib.hipk_csr_format(A) == 4
        padded = SC.padding_numpy(rp)[0]
        assert lib.hipk_csr_sliced_padding(A) == padded / len(ci)
        es, ns = np.dtype(NPDT[dt]).itemsize, (m + 63) // 64
        want = padded * (es + 2) + ns * 204 + 2 * m * es
        assert lib.hipk_csr_product_bytes(A, 0) == want and lib.hipk_csr_streamed_bytes(A) == want
        run = _Run(side, A, X)
        got = {w: run.product(0, w) for w in WIDTHS}
        again = run.product(0, 8)
        ones = {c: run.product(c, 1)[:, 0] for c in (0, 3, 7, 8, 63)}
        lib.hipk_csr_destroy(A)
    finally:
        lib.hipk_set_spmv_format(old)
        side.close()
    for w in WIDTHS:
        _within(got[w], ref[:, :w], B[:, :w], f"{name} dt={dt} width={w}")
    assert np.array_equal(again, got[8])                                  # run to run
    for c, y1 in ones.items():                                            # a column does not depend on the width of the call
        if c < 8: assert np.array_equal(got[8][:, c], y1), (name, c)
        if c < 9: assert np.array_equal(got[9][:, c], y1), (name, c)
        assert np.array_equal(got[64][:, c], y1), (name, c)
    assert np.array_equal(got[1][:, 0], ones[0]) and np.array_equal(got[3], got[64][:, :3]) and np.array_equal(got[4], got[64][:, :4])


@pytest.mark.parametrize("dt", DTYPES)
def test_padding_never_contributes(built, dt):
    npdt = NPDT[dt]
    side = Dev()
    lib = side.lib
    old = lib.hipk_set_spmv_format(1)
    results = []
    try:
        # (a) NaN where no row looks: column 0, column n - 1 and the first columns of slices 1 and 2
        rp, ci, va = SC.matrix("holes257")
        m = len(rp) - 1
        dead = [0, 64, 128, m - 1]
        assert not np.isin(ci, dead).any()
        # (b) NaN / Inf at the very columns the padding entries of the random band matrix point at: a padded slot that
        # contributed would turn a row that does not reference those columns into NaN
        rb = SC.matrix("random_band")
        rc, Sl = SC.to_sliced(checkers.load_hostcheck(), rb[0], rb[1], rb[2])
        assert rc == 0
        live = np.zeros(int(Sl.base[-1]), dtype=bool)
        for p in range(Sl.m):
            live[Sl.base[p // 64] + 64 * np.arange(Sl.len[p]) + p % 64] = True
        padcols = np.unique((Sl.idx.astype(np.int64) + np.repeat(Sl.cmin, np.diff(Sl.base)))[~live])
        assert len(padcols) > 0 and (~live).sum() > 500
        for (rp, ci, va), bad in ((SC.matrix("holes257"), np.array(dead)), (rb, padcols)):
            m = len(rp) - 1
            X = (np.random.default_rng(5).standard_normal((m, 8)) * 2.0).astype(npdt)
            Xz = X.copy(); Xz[bad] = 0.0
            X[bad[0::2]] = np.nan; X[bad[1::2]] = np.inf
            rows = np.repeat(np.arange(m), np.diff(rp))
            touched = np.zeros(m, dtype=bool); touched[rows[np.isin(ci, bad)]] = True
            A = _create(side, dt, rp, ci, va, m, 0, F.HIPK_CSR_SLICED)
            assert lib.hipk_csr_sliced(A) == 1
            run = _Run(side, A, X)
            results.append((rp, ci, va.astype(npdt), Xz, touched, bad, run.product(0, 8), run.product(0, 1), run.product(0, 8, shift=np.zeros(8))))
            lib.hipk_csr_destroy(A)
    finally:
        lib.hipk_set_spmv_format(old)
        side.close()
    for rp, ci, vt, Xz, touched, bad, y8, y1, ys in results:
        ok = ~touched
        assert ok.sum() > len(ok) // 2
        ref, S = SC.product_reference(rp, ci, vt, Xz)
        B = SC.product_bound(rp, ref, S, npdt)
        own = ok.copy(); own[bad] = False             # the shifted product (shift 0) reads the row's own x entry as well
        for y, sel in ((y8, ok), (ys, own)):
            assert np.all(np.isfinite(y[sel]))
            assert np.all(np.abs(y[sel].astype(L) - ref[sel]) <= B[sel])
        assert np.all(np.isfinite(y1[ok])) and np.array_equal(y1[ok, 0], y8[ok, 0])
        assert not np.any(np.isfinite(y8[touched]))                       # the rows that do reference those columns say so


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("name", ["lunda3", "random_band", "band65"])
def test_shifted_product(built, name, dt):
    """y = A x - shift[c] x(:, c): the shift term is one more entry of the row's chain (fma(-shift, x_i, sum)), so the bound is
    the product's with |shift| |x_i| added to sum_j |a_ij| |x_j| — (len_i + 2) covers the extra rounding"""
    rp, ci, va = SC.matrix(name)
    m = len(rp) - 1
    npdt = NPDT[dt]
    X, vt, ref, S, _ = _reference(name, dt, 64)
    shift = np.random.default_rng(77).standard_normal(9) * float(np.abs(va).max())
    side = Dev()
    lib = side.lib
    old = lib.hipk_set_spmv_format(1)
    try:
        A = _create(side, dt, rp, ci, va, m, 0, F.HIPK_CSR_SLICED)
        assert lib.hipk_csr_sliced(A) == 1
        run = _Run(side, A, X)
        got = {w: run.product(0, w, shift=shift[:w]) for w in (1, 8, 9)}
        lib.hipk_csr_destroy(A)
    finally:
        lib.hipk_set_spmv_format(old)
        side.close()
    for w, y in got.items():
        sx = shift[None, :w].astype(L) * X[:, :w].astype(L)
        r = ref[:, :w] - sx
        _within(y, r, SC.product_bound(rp, r, S[:, :w], npdt, extra=np.abs(sx)), f"shifted {name} dt={dt} width={w}")
    assert np.array_equal(got[9][:, :8], got[8]) and np.array_equal(got[8][:, :1], got[1])


@pytest.mark.parametrize("dt", DTYPES)
def test_32_bit_indices(built, dt):
    rp, ci, va = SC.matrix("wide")
    m = len(rp) - 1
    X, vt, ref, S, B = _reference("wide", dt, 8)
    side = Dev()
    lib = side.lib
    old = lib.hipk_set_spmv_format(1)
    try:
        A = _create(side, dt, rp, ci, va, m, 0, F.HIPK_CSR_SLICED)
        assert lib.hipk_csr_sliced(A) == 1 and lib.hipk_csr_format(A) == 4
        es = np.dtype(NPDT[dt]).itemsize
        assert lib.hipk_csr_product_bytes(A, 0) == SC.padding_numpy(rp)[0] * (es + 4) + ((m + 63) // 64) * 204 + 2 * m * es
        run = _Run(side, A, X)
        y8, y1 = run.product(0, 8), run.product(0, 1)
        lib.hipk_csr_destroy(A)
    finally:
        lib.hipk_set_spmv_format(old)
        side.close()
    _within(y8, ref, B, f"wide dt={dt} width=8")
    assert np.array_equal(y1[:, 0], y8[:, 0])


def _slab():
    dims = (23, 19, 17)
    row0, nloc = 2000, 3003
    rp, ci, va, _ = problems.laplacian_csr(dims, row0=row0, nrows=nloc)
    va = np.array(va, dtype=np.float64)
    va += np.random.default_rng(4).standard_normal(len(va)) * 0.25        # no two rows alike: not the row-pattern form
    return rp, ci, va, int(np.prod(dims)), row0


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("case", ["fallback300", "slab_with_halo"])
def test_fallback_and_uncovered(built, case, dt):
    npdt = NPDT[dt]
    if case == "fallback300":
        rp, ci, va = SC.matrix(case); n, row0 = len(rp) - 1, 0
    else:
        rp, ci, va, n, row0 = _slab()
    nloc = len(rp) - 1
    Xg = (np.random.default_rng(41).standard_normal((n, 8)) * 2.0).astype(npdt)
    side = Dev()
    lib = side.lib
    old = lib.hipk_set_spmv_format(1)
    got = {}
    try:
        for flags in (F.HIPK_CSR_SLICED, 0):
            A = _create(side, dt, rp, ci, va, n, row0, flags)
            assert lib.hipk_csr_sliced(A) == 0 and lib.hipk_csr_sliced_padding(A) == 0.0 and lib.hipk_csr_format(A) == 0
            lo, hi = int(lib.hipk_csr_halo_lo(A)), int(lib.hipk_csr_halo_hi(A))
            assert (lo > 0 and hi > 0) == (case == "slab_with_halo")
            xlo = side.arr(np.ascontiguousarray(Xg[row0 - lo:row0].T).ravel() if lo else np.zeros(1, npdt))
            xhi = side.arr(np.ascontiguousarray(Xg[row0 + nloc:row0 + nloc + hi].T).ravel() if hi else np.zeros(1, npdt))
            assert lib.hipk_csr_set_halo_ld(A, side.ptr(xlo), max(lo, 1), side.ptr(xhi), max(hi, 1)) == 0
            run = _Run(side, A, Xg[row0:row0 + nloc])
            got[flags] = (run.product(0, 1), run.product(0, 8), lib.hipk_csr_product_bytes(A, 0))
            lib.hipk_csr_destroy(A)
    finally:
        lib.hipk_set_spmv_format(old)
        side.close()
    a, b = got[F.HIPK_CSR_SLICED], got[0]
    assert not np.any(np.isnan(b[1]))
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and a[2] == b[2]


@pytest.mark.parametrize("dt", DTYPES)
def test_run_time_switch(built, dt):
    name = "random_band"
    rp, ci, va = SC.matrix(name)
    m = len(rp) - 1
    X, vt, ref, S, B = _reference(name, dt, 64)
    side = Dev()
    lib = side.lib
    old = lib.hipk_set_spmv_format(1)
    try:
        A = _create(side, dt, rp, ci, va, m, 0, F.HIPK_CSR_SLICED)
        run = _Run(side, A, X[:, :8])
        ys = run.product(0, 8), run.product(0, 1), run.product(0, 8, shift=np.ones(8))
        fmt4 = lib.hipk_csr_format(A)
        bytes4 = lib.hipk_csr_product_bytes(A, 0)
        assert lib.hipk_set_spmv_format(0) == 1
        assert lib.hipk_csr_format(A) == 0 and lib.hipk_csr_sliced(A) == 1 and lib.hipk_csr_streamed_bytes(A) == 0.0
        assert lib.hipk_csr_product_bytes(A, 0) != bytes4
        yt = run.product(0, 8), run.product(0, 1), run.product(0, 8, shift=np.ones(8))
        assert lib.hipk_set_spmv_format(1) == 0                           # the previous setting comes back, and restores
        assert lib.hipk_csr_format(A) == 4
        back = run.product(0, 8)
        lib.hipk_csr_destroy(A)
    finally:
        lib.hipk_set_spmv_format(old)
        side.close()
    assert fmt4 == 4 and np.array_equal(back, ys[0])
    for a, b, w in ((ys[0], yt[0], 8), (ys[1], yt[1], 1)):
        assert not np.any(np.isnan(b))
        assert np.all(np.abs(a.astype(L) - b.astype(L)) <= 2 * B[:, :w])
    Bs = SC.product_bound(rp, ref[:, :8] - X[:, :8].astype(L), S[:, :8], NPDT[dt], extra=np.abs(X[:, :8].astype(L)))
    assert np.all(np.abs(ys[2].astype(L) - yt[2].astype(L)) <= 2 * Bs)


@pytest.mark.parametrize("dt", DTYPES)
def test_unrouted_entry_points(built, dt):
    """the Chebyshev step, the fused one-column product and the Gershgorin pass read the CSR arrays of a flagged handle exactly as
    those of an unflagged one"""
    npdt = NPDT[dt]
    rp, ci, va = SC.matrix("lunda3")
    m = len(rp) - 1
    rng = np.random.default_rng(3)
    Xc, Yk, Yp = (rng.standard_normal((3, m)).astype(npdt) for _ in range(3))
    x1 = rng.standard_normal(m).astype(npdt)
    cf, _ = _coef()
    side = Dev()
    lib = side.lib
    old = lib.hipk_set_spmv_format(1)
    got = {}
    try:
        for flags in (F.HIPK_CSR_SLICED, 0):
            A = _create(side, dt, rp, ci, va, m, 0, flags)
            assert lib.hipk_csr_sliced(A) == (1 if flags else 0)
            dx, dk, dp = side.arr(Xc.ravel()), side.arr(Yk.ravel()), side.arr(Yp.ravel())
            out = side.arr(np.full(3 * m, np.nan, npdt))
            assert lib.hipk_csr_cheb_step(A, None, 3, C.byref(cf), side.ptr(dx), m, side.ptr(dk), m, side.ptr(dp), m, side.ptr(out), m) == 0
            x = side.arr(x1); nn = side.arr(np.array([float(np.sum(x1.astype(np.float64) ** 2))]))
            xo, y, dot = side.arr(np.full(m, np.nan, npdt)), side.arr(np.full(m, np.nan, npdt)), side.arr(np.zeros(1))
            assert lib.hipk_csr_matvec_scaled(A, side.ctx, side.ptr(x), side.ptr(nn), side.ptr(xo), side.ptr(y), side.ptr(dot)) == 0
            g = (C.c_double * 2)()
            assert lib.hipk_csr_gershgorin(A, None, g) == 0
            got[flags] = [side.get(t) for t in (out, xo, y, dot)] + [np.array([g[0], g[1]]), np.array([lib.hipk_csr_product_bytes(A, 1)])]
            lib.hipk_csr_destroy(A)
    finally:
        lib.hipk_set_spmv_format(old)
        side.close()
    for a, b in zip(got[F.HIPK_CSR_SLICED], got[0]):
        assert not np.any(np.isnan(b)) and np.array_equal(a, b)


@functools.lru_cache(maxsize=None)
def _lunda4():
    rp, ci, va = SC.matrix("lunda4")
    n = len(rp) - 1
    M = np.zeros((n, n)); M[np.repeat(np.arange(n), np.diff(rp)), ci] = va
    return rp, ci, va, n, np.linalg.eigvalsh(M)


def test_solve_block_jdqmr(built):
    """LUNDA x 4 (588 rows), 6 smallest, JDQMR, block size 4, Jacobi: the shifted block products go through the sliced form"""
    rp, ci, va, n, lam = _lunda4()
    assert n == 588
    eps, anorm = 1e-10, float(np.abs(lam).max())
    res = {}
    for flag in (True, False):
        r = eigsh(Operator(n, csr=(rp, ci, va), sliced=flag), numEvals=6, method="JDQMR", maxBlockSize=4, eps=eps, aNorm=anorm,
                  precond="jacobi", v0=problems.start_vector(n))
        assert r.ret == 0 and r.initSize == 6
        assert np.max(np.abs(np.sort(r.evals) - lam[:6])) <= eps * anorm, (flag, r.evals, lam[:6])
        assert np.all(r.resNorms <= eps * anorm * (1 + 1e-6)), (flag, r.resNorms)
        res[flag] = (np.sort(r.evals), r.stats["numOuterIterations"], r.stats["numMatvecs"])
    print("outer iterations / matvecs with and without the form:", res[True][1:], res[False][1:])
    assert np.max(np.abs(res[True][0] - res[False][0])) <= eps * anorm
    for k in (1, 2):
        assert abs(res[True][k] - res[False][k]) <= BAND * max(res[True][k], res[False][k]), res


def test_solve_gd_plusk_block_1(built):
    rp, ci, va, n, lam = _lunda4()
    eps, anorm = 1e-9, float(np.abs(lam).max())
    for flag in (True, False):
        r = eigsh(Operator(n, csr=(rp, ci, va), sliced=flag), numEvals=3, method="GD_plusK", maxBlockSize=1, eps=eps, aNorm=anorm,
                  precond="jacobi", v0=problems.start_vector(n))
        assert r.ret == 0 and r.initSize == 3
        assert np.max(np.abs(np.sort(r.evals) - lam[:3])) <= eps * anorm, (flag, r.evals, lam[:3])
        assert np.all(r.resNorms <= eps * anorm * (1 + 1e-6)), (flag, r.resNorms)


def test_python_keyword_reaches_the_form(built):
    rp, ci, va, n, _ = _lunda4()
    for kw, want in ((dict(sliced=True), 1), (dict(), 0), (dict(sliced=True, diag_patterns=True), 1)):
        s = Session(Operator(n, csr=(rp, ci, va), **kw))
        try:
            A = dict((k, h) for k, h in s.handles)["csr"]
            assert s.lib.hipk_csr_sliced(A) == want and s.lib.hipk_csr_format(A) == (4 if want else 0)
        finally:
            s.close()
