"""The two kernels the singular value solver's Chebyshev preconditioner adds: hipk_csr_cheb_step_gather (the recurrence step as
an epilogue of the windowed tile kernel for a RECTANGULAR matrix, csrc/hipk_sparse.hip) and hipk_csr_abs_rowsum_max
(csrc/hipk_cheb.hip), with the panel discipline of test_cheb_kernels_gpu.py: NaN everywhere outside the block, padding rows and
the column behind the block unchanged bit for bit, inputs unchanged, distinct odd leading dimensions (some columns are only
8-byte aligned).

Bound per element, as there: |out_i - ref_i| <= u_T |ref_i| + 2 (len_i + 4) 2^-53 S_i against np.longdouble, S_i the sum of the
absolute values of everything that is added for row i.  In double the step also equals hipk_csr_matvec (all nx columns at once)
followed by hipk_cheb_update bit for bit: the kernel forms the row sum the way the product forms it for that matrix and width.

  band_70001x50003   rows no multiple of a tile, 2 and 3 entries per row, windowed tiles, 16-bit indices
  band_50003x70001   more columns than rows
  wide32_rect        two entries per row 66 000 columns apart: the 4-byte index stream, gather tiles, not windowed (the plain
                     products of nx >= 2 run the row-block kernel: no two-lane split)
  empty_rows         every third row empty and a stretch of 700 empty rows (tiles without a nonzero)
  long_row           a 4000-entry row (nz > TILE_NNZ: the long-row branch) in a windowed band matrix
  long_row_wide32    the same in a matrix that is not windowed (the row-block kernel's long-row branch is the pair's)
  nx = 1 (the one-column product's rounded products), 3 and 8; Out apart, Out == Yprev, Out == Yk, Yprev NULL, Yk NULL."""
import ctypes as C

import numpy as np
import pytest

import svds_cheb_cases as SC
from kernel_harness import Dev, NPDT
from primme_amd import _ffi as F
from primme_amd import problems
from test_cheb_kernels_gpu import L, _Panel, _coef, _declare, _u, num_cu  # noqa: F401

pytestmark = pytest.mark.gpu
CASES = ["band_70001x50003", "band_50003x70001", "wide32_rect", "empty_rows", "long_row", "long_row_wide32"]
VARIANTS = ("apart", "out_is_yprev", "out_is_yk", "no_yprev", "no_yk")


def _band(m, n, seed, keep_row=None):
    """row i: 2 (i even) or 3 (i odd) entries at consecutive columns around i n / m"""
    rng = np.random.default_rng(seed)
    i = np.arange(m)
    c0 = np.minimum((i * n) // m, n - 3)
    cols = np.stack([c0, c0 + 1, c0 + 2], axis=1)
    keep = np.ones((m, 3), dtype=bool)
    keep[::2, 2] = False
    if keep_row is not None:
        keep &= keep_row[:, None]
    rp = np.zeros(m + 1, dtype=np.int32)
    np.cumsum(keep.sum(axis=1), out=rp[1:])
    return rp, cols[keep].astype(np.int32), rng.standard_normal(int(keep.sum()))


def _case(name):
    if name == "band_70001x50003":
        return (70001, 50003) + _band(70001, 50003, 1)
    if name == "band_50003x70001":
        return (50003, 70001) + _band(50003, 70001, 2)
    if name == "wide32_rect":
        m, n = 70001, 80021
        rng = np.random.default_rng(5)
        i = np.arange(m)
        ci = np.sort(np.stack([i, (i + 66000) % n], axis=1), axis=1).reshape(-1).astype(np.int32)
        return m, n, np.arange(0, 2 * m + 1, 2, dtype=np.int32), ci, rng.standard_normal(2 * m)
    if name in ("long_row", "long_row_wide32"):
        # one row of 4000 entries: a tile of its own (nz > TILE_NNZ), summed by the whole workgroup — strided fma, wave sums, a
        # fixed tree — in the one-column, the windowed and the row-block product alike
        m, n = (5003, 9001) if name == "long_row" else (20001, 80021)
        if name == "long_row":
            rp, ci, va = _band(m, n, 7)
        else:
            i = np.arange(m)
            ci = np.sort(np.stack([i, (i + 66000) % n], axis=1), axis=1).reshape(-1).astype(np.int32)
            rp, va = np.arange(0, 2 * m + 1, 2, dtype=np.int32), np.random.default_rng(8).standard_normal(2 * m)
        r = 1234
        cnt = np.diff(rp)
        cnt[r] = 4000
        rp2 = np.concatenate([[0], np.cumsum(cnt)]).astype(np.int32)
        ci2 = np.concatenate([ci[:rp[r]], (2 * np.arange(4000) + 5).astype(np.int32), ci[rp[r + 1]:]])
        va2 = np.concatenate([va[:rp[r]], np.random.default_rng(9).standard_normal(4000), va[rp[r + 1]:]])
        return m, n, rp2, ci2, va2
    m, n = 30011, 20011
    keep = np.arange(m) % 3 != 0
    keep[9000:9700] = False
    return (m, n) + _band(m, n, 3, keep_row=keep)


def _create_rect(side, dt, m, n, rp, ci, va):
    A = C.c_void_p()
    rp, ci = np.ascontiguousarray(rp, dtype=np.int32), np.ascontiguousarray(ci, dtype=np.int32)
    vv = np.ascontiguousarray(va, dtype=NPDT[dt])
    assert side.lib.hipk_csr_create_rect(side.ctx, dt, m, n, rp.ctypes.data_as(C.c_void_p), ci.ctypes.data_as(C.c_void_p),
                                         vv.ctypes.data_as(C.c_void_p), C.byref(A)) == 0
    return A


def _reference(m, rp, ci, vat, G, Yk, Yp, X, coefs):
    """ref and S in np.longdouble for all 8 columns, keyed by (Yk present, Yprev present)"""
    cy, cp, cx, cw = (np.asarray(c).astype(L) for c in coefs)
    g, yk, yp, x = G.astype(L), Yk.astype(L), Yp.astype(L), X.astype(L)
    prod = vat.astype(L)[:, None] * g[ci]
    AG, aAG = np.zeros((m, 8), dtype=L), np.zeros((m, 8), dtype=L)
    ne = np.diff(rp) > 0
    AG[ne] = np.add.reduceat(prod, rp[:-1][ne], axis=0)
    aAG[ne] = np.add.reduceat(np.abs(prod), rp[:-1][ne], axis=0)
    out = {}
    for hk in (True, False):
        for hp in (True, False):
            ref, S = cx * x + cw * AG, np.abs(cx) * np.abs(x) + np.abs(cw) * aAG
            if hk: ref, S = ref + cy * yk, S + np.abs(cy) * np.abs(yk)
            if hp: ref, S = ref + cp * yp, S + np.abs(cp) * np.abs(yp)
            out[hk, hp] = (ref, S)
    return out


@pytest.mark.parametrize("dt", [F.HIPK_F64, F.HIPK_F32])
@pytest.mark.parametrize("case", CASES)
def test_gather_step(built, case, dt):
    m, n, rp, ci, va = _case(case)
    npdt = NPDT[dt]
    side = Dev()
    lib = side.lib
    _declare(lib)
    try:
        A = _create_rect(side, dt, m, n, rp, ci, va)
        assert lib.hipk_csr_format(A) == 0
        assert lib.hipk_csr_index_bytes(A) == (4 if "wide32" in case else 2)
        rng = np.random.default_rng(m + 11)
        G = rng.standard_normal((n, 8)).astype(npdt)
        Yk, Yp, X = (rng.standard_normal((m, 8)).astype(npdt) for _ in range(3))
        cf, coefs = _coef()
        refs = _reference(m, rp, ci, np.asarray(va).astype(npdt), G, Yk, Yp, X, coefs)
        lens = np.diff(rp).astype(L)[:, None]
        ldx, ldk, ldp, ldo, ldw, ldq, ldg = m + 2, m + 4, m + 6, m + 8, m + 10, m + 12, n + 2
        assert all(v % 2 == 1 for v in (ldx, ldk, ldp, ldo, ldw, ldq, ldg))
        st = lib.hipk_ctx_stream(side.ctx)
        worst = 0.0
        for nx in (1, 3, 8):
            px, pg = _Panel(side, X[:, :nx], ldx), _Panel(side, G[:, :nx], ldg)
            for variant in VARIANTS:
                pk = _Panel(side, Yk[:, :nx], ldk) if variant != "no_yk" else None
                pp = _Panel(side, Yp[:, :nx], ldp) if variant != "no_yprev" else None
                tag = f"{case} {np.dtype(npdt).name} nx={nx} {variant}"
                # the pair the step replaces, first (the aliased variants overwrite an input afterwards)
                pw, pq = _Panel(side, None, ldw, shape=(m, nx, npdt)), _Panel(side, None, ldq, shape=(m, nx, npdt))
                assert lib.hipk_csr_matvec(A, None, pg.ptr, ldg, pw.ptr, ldw, nx) == 0
                assert lib.hipk_cheb_update(st, dt, m, nx, C.byref(cf), px.ptr, ldx, pw.ptr, ldw, pk.ptr if pk else None, ldk,
                                            pp.ptr if pp else None, ldp, pq.ptr, ldq) == 0
                pair = pq.read()[0]
                po, lo = {"out_is_yprev": (pp, ldp), "out_is_yk": (pk, ldk)}.get(variant, (None, ldo))
                if po is None:
                    po = _Panel(side, None, ldo, shape=(m, nx, npdt))
                assert lib.hipk_csr_cheb_step_gather(A, None, nx, C.byref(cf), px.ptr, ldx, pg.ptr, ldg, pk.ptr if pk else None, ldk,
                                                     pp.ptr if pp else None, ldp, po.ptr, lo) == 0
                out, raw = po.read()
                assert not np.any(np.isnan(out)), tag
                assert po.outside_unchanged(raw), tag
                assert px.unchanged() and pg.unchanged(), tag
                assert pk is None or po is pk or pk.unchanged(), tag
                assert pp is None or po is pp or pp.unchanged(), tag
                ref, S = refs[pk is not None, pp is not None]
                ref, S = ref[:, :nx], S[:, :nx]
                B = _u(npdt) * np.abs(ref) + 2 * (lens + 4) * L(2.0) ** -53 * S
                err = np.abs(out.astype(L) - ref)
                ratio = float(np.max(np.where(B > 0, err / np.where(B > 0, B, 1), np.where(err > 0, np.inf, 0))))
                print(f"{tag}: err/B = {ratio:.3f}  equal to the pair: {np.array_equal(pair, out)}")
                worst = max(worst, ratio)
                assert np.all(err <= B), (tag, ratio)
                if dt == F.HIPK_F64:
                    assert np.array_equal(pair, out), tag
        print(f"{case} {np.dtype(npdt).name}: max err/B = {worst:.4f}")
        lib.hipk_csr_destroy(A)
    finally:
        side.close()


def test_gather_step_return_codes(built):
    """1 = no row-tile form (panel-blocked, stencil, complex); -1 = nx = 9, Out == G, NULL X; 0 with nothing written for nx = 0."""
    side = Dev()
    lib = side.lib
    _declare(lib)
    cf, _ = _coef()
    m, n, ld = 600, 500, 700
    rng = np.random.default_rng(1)
    px, pk, pp = (_Panel(side, rng.standard_normal((m, 9)), ld) for _ in range(3))
    pg = _Panel(side, rng.standard_normal((n, 9)), ld)
    po = _Panel(side, None, ld, shape=(m, 9, np.float64))

    def step(A, nx, x, g, out):
        return lib.hipk_csr_cheb_step_gather(A, None, nx, C.byref(cf), x.ptr if x else None, ld, g.ptr, ld, pk.ptr, ld, pp.ptr, ld, out.ptr, ld)
    try:
        made = []
        # panel-blocked: x larger than an XCD's L2, a million scattered entries
        M, N = 600000, 800000
        ci = rng.integers(0, N, size=2 * M).astype(np.int32)
        made.append(_create_rect(side, F.HIPK_F64, M, N, np.arange(0, 2 * M + 1, 2, dtype=np.int32), ci, np.ones(2 * M)))
        assert lib.hipk_csr_format(made[-1]) == 1
        assert step(made[-1], 2, px, pg, po) == 1
        A = C.c_void_p()
        assert lib.hipk_stencil_create(side.ctx, F.HIPK_F64, 20, 30, 1, 0, m, C.byref(A)) == 0
        made.append(A)
        assert step(A, 2, px, pg, po) == 1
        rp, ci, va = problems.hermitian_banded_csr(m)[:3]
        A = C.c_void_p()
        assert lib.hipk_csr_create(side.ctx, F.HIPK_C64, m, m, 0, np.ascontiguousarray(rp, dtype=np.int32).ctypes.data_as(C.c_void_p),
                                   np.ascontiguousarray(ci, dtype=np.int32).ctypes.data_as(C.c_void_p),
                                   np.ascontiguousarray(va, dtype=np.complex128).ctypes.data_as(C.c_void_p), C.byref(A)) == 0
        made.append(A)
        assert step(A, 2, px, pg, po) == 1
        rp, ci, va = _band(m, n, 4)
        A = _create_rect(side, F.HIPK_F64, m, n, rp, ci, va)
        made.append(A)
        assert lib.hipk_csr_format(A) == 0
        assert step(A, 9, px, pg, po) == -1
        assert step(A, 2, px, po, po) == -1
        assert step(A, 2, None, pg, po) == -1
        assert step(A, 0, px, pg, po) == 0
        assert po.unchanged() and pp.unchanged() and pk.unchanged() and pg.unchanged()
        assert step(A, 2, px, pg, po) == 0
        assert not np.any(np.isnan(po.read()[0][:, :2]))
        for A in made:
            lib.hipk_csr_destroy(A)
    finally:
        side.close()


# ---- hipk_csr_abs_rowsum_max --------------------------------------------------------------------------------------------
def _rowsum_numpy(m, rp, va, npdt):
    a = np.abs(np.asarray(va).astype(npdt).astype(np.float64))
    rows = np.repeat(np.arange(m), np.diff(rp))
    return float(np.max(np.bincount(rows, weights=a, minlength=m))) if m and len(a) else 0.0


def _eighths(m, n, heavy_row, per_row=2):
    """per_row entries per row, multiples of 1/8 (every sum is exact in float and double); one row carries the maximum"""
    i = np.arange(m)
    ci = np.sort(np.stack([(i * 7 + 3 * j) % n for j in range(per_row)], axis=1), axis=1).reshape(-1).astype(np.int32)
    va = np.stack([((-1.0) ** (i + j)) * (1 + (i + j) % 5) / 8.0 for j in range(per_row)], axis=1)
    va[heavy_row] = -40.0
    return np.arange(0, per_row * m + 1, per_row, dtype=np.int32), ci, va.reshape(-1)


@pytest.mark.parametrize("dt", [F.HIPK_F64, F.HIPK_F32])
def test_abs_rowsum_max(built, num_cu, dt):  # noqa: F811
    npdt = NPDT[dt]
    side = Dev()
    lib = side.lib
    try:
        cases = []
        m, n, (rp, ci, va) = SC.difference_matrix(200)
        cases.append(("D", m, n, rp, ci, va, 2.0))
        m, n = 3 * 256 + 57, 500                               # the heavy row in the last, partial tile
        cases.append(("heavy row in the last tile", m, n) + _eighths(m, n, m - 2) + (80.0,))
        m, n = num_cu * 8 * 256 + 1000 * 256 + 77, 4001        # more rows than the capped grid has lanes: the maximum in a second trip
        cases.append(("larger than one grid pass", m, n) + _eighths(m, n, m - 1) + (80.0,))
        cases.append(("no entries", 300, 200, np.zeros(301, dtype=np.int32), np.zeros(1, dtype=np.int32), np.zeros(1), 0.0))
        cases.append(("no rows", 0, 200, np.zeros(1, dtype=np.int32), np.zeros(1, dtype=np.int32), np.zeros(1), 0.0))
        for name, m, n, rp, ci, va, want in cases:
            A = _create_rect(side, dt, m, n, rp, ci, va)
            out = C.c_double(-1.0)
            assert lib.hipk_csr_abs_rowsum_max(A, None, C.byref(out)) == 0, name
            assert out.value == _rowsum_numpy(m, rp, va, npdt) == want, (name, out.value)
            lib.hipk_csr_destroy(A)
        # values that are no multiples of a power of two: the entries of a row are added in row order, in double
        m, n = 5003, 4001
        rp, ci, va = _band(m, n, 9)
        A = _create_rect(side, dt, m, n, rp, ci, va)
        a = np.abs(va.astype(npdt).astype(np.float64))
        want = 0.0
        for i in range(m):
            t = 0.0
            for v in a[rp[i]:rp[i + 1]]:
                t += float(v)
            want = max(want, t)
        out = C.c_double(-1.0)
        assert lib.hipk_csr_abs_rowsum_max(A, None, C.byref(out)) == 0
        assert out.value == want
        lib.hipk_csr_destroy(A)
    finally:
        side.close()
