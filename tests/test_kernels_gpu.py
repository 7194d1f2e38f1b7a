"""Kernel-level parity: every HIP entry point of include/primme_amd_kernels.h against the
plain-C restatement oracle/hipk_cpu.c on the same seeded inputs (-m gpu).

Tolerances: reductions differ from the oracle only by summation order, so they are
compared at 1e-12 relative to sum|terms| (double) / 1e-5 (float); element-wise outputs
of the update kernels at a few ulps."""
import ctypes as C
import numpy as np
import pytest

from primme_amd import _ffi as F
from primme_amd import problems
from kernel_harness import Dev, Host, segs_array, NPDT
from csr_cases import csr_cases as _csr_cases
import checkers

pytestmark = pytest.mark.gpu

SHAPES = [(1000, 5, 3), (70001, 15, 10), (300007, 41, 20), (20011, 170, 60)]


def _panels(rng, m, k, L, dt, ld_pad=3):
    npdt = NPDT[dt]
    ld = m + ld_pad
    V = rng.standard_normal((k + 8, ld)).astype(npdt)   # row j = column j (ld apart)
    Q = rng.standard_normal((max(L, 1), ld + 5)).astype(npdt)
    return V, ld, Q, ld + 5


@pytest.mark.parametrize("dt", [F.HIPK_F64, F.HIPK_F32])
@pytest.mark.parametrize("m,k,L", SHAPES)
@pytest.mark.parametrize("nx", [1, 2, 3, 8, 11])
def test_panel_dots(built, dt, m, k, L, nx):
    rng = np.random.default_rng(m + k + nx)
    V, ld, Q, ldq = _panels(rng, m, k, L, dt)
    X = rng.standard_normal((nx, ld)).astype(NPDT[dt])
    outs = []
    for side in (Dev(), Host()):
        v, q, x = side.arr(V), side.arr(Q), side.arr(X)
        out = side.arr(np.zeros((nx, k + L + 2)))
        segs = segs_array(side, [(v, 0, ld, k), (q, 0, ldq, L), (x, 0, ld, 1)])
        rc = side.lib.hipk_panel_dots(side.ctx, dt, m, segs, 3, side.ptr(x), ld, nx, side.ptr(out), k + L + 2)
        assert rc == 0
        outs.append(side.get(out)[:, :k + L + 1])
        side.close()
    scale = np.sqrt(m) * 4
    tol = (1e-12 if dt == F.HIPK_F64 else 2e-5) * scale
    assert np.max(np.abs(outs[0] - outs[1])) <= tol * max(1.0, np.abs(outs[1]).max() / scale)


@pytest.mark.parametrize("dt", [F.HIPK_F64, F.HIPK_F32])
@pytest.mark.parametrize("m,k,L,nx", [(128 * 7, 5, 0, 4), (100003, 12, 4, 8), (100003, 17, 0, 4), (70001, 24, 9, 8), (250000, 41, 8, 8),
                                      (33333, 30, 40, 16), (50001, 9, 3, 20), (90, 6, 2, 5), (257, 16, 0, 16)])
def test_panel_dots_matrix_cores(built, dt, m, k, L, nx, monkeypatch):
    """Blocks of >= 4 right-hand columns with 16-byte aligned panels go through v_mfma_f64_16x16x4_f64
    (dots_mfma_kernel): against the oracle, against numpy in float64 and against the FMA kernels
    (HIPK_NO_MFMA is read once per process, so the FMA leg is the oracle + numpy comparison here).  The
    operands are asymmetric (a row <-> column swap in the C/D layout would not cancel)."""
    rng = np.random.default_rng(m + k + nx)
    npdt = NPDT[dt]
    ld = (m + 2) // 2 * 2 + 2                       # even: every column 16-byte aligned
    V = rng.standard_normal((k + 1, ld)).astype(npdt) * np.linspace(0.5, 2.0, k + 1)[:, None].astype(npdt)
    Q = rng.standard_normal((max(L, 1), ld)).astype(npdt)
    X = (rng.standard_normal((nx, ld)) * np.linspace(1.0, 3.0, nx)[:, None]).astype(npdt)
    outs = []
    for side in (Dev(), Host()):
        v, q, x = side.arr(V), side.arr(Q), side.arr(X)
        out = side.arr(np.zeros((nx, k + L + 3)))
        segs = segs_array(side, [(q, 0, ld, L), (v, 0, ld, k)])
        assert side.lib.hipk_panel_dots(side.ctx, dt, m, segs, 2, side.ptr(x), ld, nx, side.ptr(out), k + L + 3) == 0
        outs.append(side.get(out)[:, :k + L])
        side.close()
    ref = X[:, :m].astype(np.float64) @ np.concatenate([Q[:L, :m], V[:k, :m]]).astype(np.float64).T
    scale = np.sqrt(m) * 8
    tol = (1e-12 if dt == F.HIPK_F64 else 2e-5) * scale
    assert np.max(np.abs(outs[0] - outs[1])) <= tol * max(1.0, np.abs(outs[1]).max() / scale)
    assert np.max(np.abs(outs[0] - ref)) <= tol * max(1.0, np.abs(ref).max() / scale)


@pytest.mark.parametrize("dt", [F.HIPK_F64, F.HIPK_F32])
@pytest.mark.parametrize("m,k,L", SHAPES)
@pytest.mark.parametrize("nx", [1, 2, 5, 8, 9])
def test_panel_project(built, dt, m, k, L, nx):
    rng = np.random.default_rng(7 * m + k + nx)
    V, ld, Q, ldq = _panels(rng, m, k, L, dt)
    X = rng.standard_normal((nx, ld)).astype(NPDT[dt])
    coef = rng.standard_normal((nx, k + L + 3)) / (k + L)
    res = []
    for side in (Dev(), Host()):
        v, q, x, cf = side.arr(V), side.arr(Q), side.arr(X), side.arr(coef)
        n2 = side.arr(np.zeros(nx))
        segs = segs_array(side, [(v, 0, ld, k), (q, 0, ldq, L)])
        rc = side.lib.hipk_panel_project(side.ctx, dt, m, segs, 2, side.ptr(cf), k + L + 3, side.ptr(x), ld, nx, side.ptr(n2))
        assert rc == 0
        res.append((side.get(x)[:, :m], side.get(n2)))
        side.close()
    tol = 1e-13 if dt == F.HIPK_F64 else 1e-5
    assert np.max(np.abs(res[0][0] - res[1][0])) <= tol * 10
    assert np.allclose(res[0][1], res[1][1], rtol=tol * 100)
    # rows beyond m (padding of the leading dimension) must be untouched
    # (checked implicitly: only [:m] is written by the oracle as well)


@pytest.mark.parametrize("dt", [F.HIPK_F64, F.HIPK_F32])
@pytest.mark.parametrize("m,k", [(999, 3), (50003, 15), (200001, 33), (40000, 41), (30011, 140), (5000, 255)])
def test_ritz_update_inplace_restart(built, dt, m, k):
    """The restart shape: V,W <- V h, W h in place + next block X,R + locked copies + norms."""
    rng = np.random.default_rng(m + k)
    npdt = NPDT[dt]
    ld = m + 1
    K = k + 6
    V = rng.standard_normal((K, ld)).astype(npdt)
    W = rng.standard_normal((K, ld)).astype(npdt)
    E = np.zeros((4, ld), dtype=npdt)
    h = np.linalg.qr(rng.standard_normal((k, k)))[0]
    hfull = np.zeros((k, K + 2))
    hfull[:, :k] = h.T            # row c = coefficient column c (leading dim K+2)
    theta = rng.standard_normal(k)
    rs = max(1, k // 2)
    nb = min(2, k - rs) if k > rs else 0
    nlock = min(3, k - rs)
    jobs = []
    for c in range(rs): jobs.append((F.HIPK_JOB_XV, c, ("V", c), -1))
    for c in range(nb): jobs.append((F.HIPK_JOB_XV, c, ("V", rs + nlock + c), -1))
    for c in range(nlock): jobs.append((F.HIPK_JOB_XV, rs + c, ("E", c), -1))
    for c in range(rs): jobs.append((F.HIPK_JOB_XW, c, ("W", c), -1))
    for c in range(nb): jobs.append((F.HIPK_JOB_RES, c, ("W", rs + nlock + c), c))
    for c in range(nlock): jobs.append((F.HIPK_JOB_RES, rs + c, None, nb + c))
    res = []
    for side in (Dev(), Host()):
        v, w, e, hh, th = side.arr(V), side.arr(W), side.arr(E), side.arr(hfull), side.arr(theta)
        n2 = side.arr(np.zeros(nb + nlock + 1))
        base = {"V": v, "W": w, "E": e}
        arr = (F.HipkJob * len(jobs))()
        for i, (kind, col, dst, slot) in enumerate(jobs):
            arr[i].kind, arr[i].col, arr[i].slot = kind, col, slot
            arr[i].dst = None if dst is None else side.ptr(base[dst[0]], dst[1] * ld).value
        rc = side.lib.hipk_ritz_update(side.ctx, dt, m, side.ptr(v), side.ptr(w), ld, k, side.ptr(hh), K + 2,
                                       side.ptr(th), arr, len(jobs), side.ptr(n2))
        assert rc == 0
        res.append((side.get(v), side.get(w), side.get(e), side.get(n2)))
        side.close()
    tol = 1e-12 if dt == F.HIPK_F64 else 1e-4
    for a, b in zip(res[0][:3], res[1][:3]):
        assert np.max(np.abs(a - b)) <= tol * 10
    assert np.allclose(res[0][3][:nb + nlock], res[1][3][:nb + nlock], rtol=tol * 100)


@pytest.mark.parametrize("dt", [F.HIPK_F64, F.HIPK_F32])
def test_ritz_update_many_residuals(built, dt):
    """more than 4 residual columns exercises the 16-accumulator kernel variant"""
    rng = np.random.default_rng(3)
    npdt = NPDT[dt]
    m, k, ld = 30011, 20, 30016
    V = rng.standard_normal((k + 12, ld)).astype(npdt)
    W = rng.standard_normal((k + 12, ld)).astype(npdt)
    h = rng.standard_normal((k, k))
    theta = rng.standard_normal(k)
    jobs = [(F.HIPK_JOB_RES, c, ("W", k + c) if c < 8 else None, c) for c in range(12)]
    res = []
    for side in (Dev(), Host()):
        v, w, hh, th = side.arr(V), side.arr(W), side.arr(h), side.arr(theta)
        n2 = side.arr(np.zeros(12))
        arr = (F.HipkJob * len(jobs))()
        for i, (kind, col, dst, slot) in enumerate(jobs):
            arr[i].kind, arr[i].col, arr[i].slot = kind, col, slot
            arr[i].dst = None if dst is None else side.ptr(w, dst[1] * ld).value
        rc = side.lib.hipk_ritz_update(side.ctx, dt, m, side.ptr(v), side.ptr(w), ld, k, side.ptr(hh), k,
                                       side.ptr(th), arr, len(jobs), side.ptr(n2))
        assert rc == 0
        res.append((side.get(w), side.get(n2)))
        side.close()
    tol = 1e-12 if dt == F.HIPK_F64 else 1e-4
    assert np.max(np.abs(res[0][0] - res[1][0])) <= tol * 20
    assert np.allclose(res[0][1], res[1][1], rtol=tol * 100)


@pytest.mark.parametrize("dt", [F.HIPK_F64, F.HIPK_F32])
@pytest.mark.parametrize("m,k,L,wtr,pads", [(1001, 1, 0, 0, (2, 5)), (70001, 7, 3, 0, (2, 5)), (250000, 15, 10, 0, (2, 5)), (99999, 30, 20, 0, (2, 5)),
                                            (1001, 1, 0, 1, (2, 5)), (70001, 7, 3, 1, (2, 5)), (250000, 15, 10, 1, (2, 5)), (120000, 16, 16, 1, (2, 5)),
                                            # 16-byte aligned columns (two rows per lane), ragged tails, every column-per-wave width
                                            (250000, 15, 10, 1, (2, 6)), (99999, 30, 20, 1, (1, 3)), (64 * 2 * 5 + 77, 9, 0, 1, (1, 1)),
                                            (130001, 21, 32, 1, (1, 5)), (130001, 32, 5, 0, (3, 3)), (50, 3, 2, 1, (0, 0)), (128, 6, 9, 0, (0, 0))])
def test_ritz_residual_overlaps(built, dt, m, k, L, wtr, pads):
    """fused residual + first Gram-Schmidt pass: r = W h - theta V h, out = [V'r | Q'r | r'r (| W'r | W(:,k-1)'Q)]"""
    rng = np.random.default_rng(m + k + L)
    npdt = NPDT[dt]
    ld, ldq = m + pads[0], m + pads[1]
    V = rng.standard_normal((k + 1, ld)).astype(npdt)
    W = rng.standard_normal((k + 1, ld)).astype(npdt)
    Q = rng.standard_normal((max(L, 1), ldq)).astype(npdt)
    h = rng.standard_normal(k) / np.sqrt(k)
    theta = 0.37
    res = []
    for side in (Dev(), Host()):
        v, w, q, hh = side.arr(V), side.arr(W), side.arr(Q), side.arr(h)
        out = side.arr(np.zeros(k + L + 1 + (k + L if wtr else 0)))
        hhost = np.ascontiguousarray(h)
        rc = side.lib.hipk_ritz_residual_overlaps(side.ctx, dt, m, side.ptr(v), side.ptr(w), ld, k, hhost.ctypes.data_as(C.c_void_p),
                                                  C.c_double(theta), side.ptr(v, k * ld), side.ptr(q), ldq, L, wtr, side.ptr(out))
        assert rc == 0
        res.append((side.get(v)[k, :m], side.get(out)))
        side.close()
    if wtr:
        r = res[1][0].astype(np.float64)
        assert np.allclose(res[1][1][2 * k + L + 1:], Q[:L, :m].astype(np.float64) @ W[k - 1, :m].astype(np.float64), rtol=1e-3 if dt == F.HIPK_F32 else 1e-9, atol=1e-6 * np.sqrt(m))
        assert np.allclose(res[1][1][k + L + 1:2 * k + L + 1], W[:k, :m].astype(np.float64) @ r, rtol=1e-3 if dt == F.HIPK_F32 else 1e-9, atol=1e-6 * np.sqrt(m))
    tol = 1e-12 if dt == F.HIPK_F64 else 1e-4
    assert np.max(np.abs(res[0][0] - res[1][0])) <= tol * 10
    scale = np.sqrt(m) * 4
    assert np.max(np.abs(res[0][1] - res[1][1])) <= tol * scale * max(1.0, np.abs(res[1][1]).max() / scale)


@pytest.mark.parametrize("dt", [F.HIPK_F64, F.HIPK_F32])
@pytest.mark.parametrize("m,k,nb,L,inplace", [(70001, 15, 8, 0, True), (70001, 15, 8, 5, True), (250003, 15, 8, 10, False),
                                              (33333, 7, 3, 2, True), (50001, 30, 16, 20, False), (20000, 16, 9, 32, True),
                                              (999, 2, 1, 1, True)])
def test_ritz_update_overlaps(built, dt, m, k, nb, L, inplace):
    """restart pass + residual of the next candidate + its inner products with the basis being written:
    ov = [(V h)'r | Q'r | r'r | (W h)'r | W(:,k-1)'Q], in place (the restart) and out of place"""
    rng = np.random.default_rng(m + 7 * k + L)
    npdt = NPDT[dt]
    ld, ldq = m + 2, m + 5
    V = (rng.standard_normal((2 * k + 2, ld)) / np.sqrt(m)).astype(npdt)
    W = (rng.standard_normal((2 * k + 2, ld)) / np.sqrt(m)).astype(npdt)
    Q = (rng.standard_normal((max(L, 1), ldq)) / np.sqrt(m)).astype(npdt)
    h = rng.standard_normal((k, k)) / np.sqrt(k)
    theta = rng.standard_normal(k)
    off = 0 if inplace else k + 1            # destination columns
    rescol = nb if nb < k else k - 1
    jobs = [(F.HIPK_JOB_XV, c, ("V", off + c), -1) for c in range(nb)]
    jobs += [(F.HIPK_JOB_XV, k - 1, ("V", 2 * k + 1), -1)]                      # one more output that is not a basis column
    jobs += [(F.HIPK_JOB_XW, c, ("W", off + c), -1) for c in range(nb)]
    jobs += [(F.HIPK_JOB_RES, rescol, ("W", 2 * k), 0)]
    res = []
    for side in (Dev(), Host()):
        v, w, q, hh, th = side.arr(V), side.arr(W), side.arr(Q), side.arr(h), side.arr(theta)
        n2 = side.arr(np.zeros(2)); ov = side.arr(np.zeros(2 * nb + 2 * L + 1))
        arr = (F.HipkJob * len(jobs))()
        for i, (kind, col, dst, slot) in enumerate(jobs):
            arr[i].kind, arr[i].col, arr[i].slot = kind, col, slot
            arr[i].dst = side.ptr(v if dst[0] == "V" else w, dst[1] * ld).value
        rc = side.lib.hipk_ritz_update_overlaps(side.ctx, dt, m, side.ptr(v), side.ptr(w), ld, k, side.ptr(hh), k, side.ptr(th),
                                                arr, len(jobs), side.ptr(n2), nb, side.ptr(q), ldq, L, side.ptr(ov))
        assert rc == 0
        res.append((side.get(v)[:, :m], side.get(w)[:, :m], side.get(n2), side.get(ov)))
        side.close()
    # the checker against numpy on the same inputs
    Vd, Wd, Qd = V[:, :m].astype(np.float64), W[:, :m].astype(np.float64), Q[:L, :m].astype(np.float64)
    r = res[1][1][2 * k]
    assert np.allclose(r, (h[rescol] @ Wd[:k]) - theta[rescol] * (h[rescol] @ Vd[:k]), atol=1e-5 if dt == F.HIPK_F32 else 1e-13)   # column c of the C array = h[c]
    exp = np.concatenate([res[1][0][off:off + nb] @ r, Qd @ r, [r @ r], res[1][1][off:off + nb] @ r, Qd @ Wd[k - 1]])
    assert np.allclose(res[1][3], exp, rtol=1e-3 if dt == F.HIPK_F32 else 1e-9, atol=1e-7)
    tol = 1e-12 if dt == F.HIPK_F64 else 1e-4
    assert np.max(np.abs(res[0][0] - res[1][0])) <= tol and np.max(np.abs(res[0][1] - res[1][1])) <= tol
    assert np.allclose(res[0][2][0], res[1][2][0], rtol=tol * 100)
    assert np.max(np.abs(res[0][3] - res[1][3])) <= tol * 10 * max(1.0, np.abs(res[1][3]).max())


@pytest.mark.parametrize("dt", [F.HIPK_F64, F.HIPK_F32])
def test_column_utilities(built, dt):
    rng = np.random.default_rng(11)
    npdt = NPDT[dt]
    m, ld, nx = 123457, 123460, 5
    X = rng.standard_normal((nx, ld)).astype(npdt)
    Y = rng.standard_normal((nx, ld)).astype(npdt)
    alpha = rng.standard_normal(nx)
    perm = np.array([3, 0, 4, 1, 2], dtype=np.int32)
    res = []
    for side in (Dev(), Host()):
        x, y = side.arr(X), side.arr(Y)
        z = side.arr(np.zeros_like(X))
        n2 = side.arr(np.zeros(nx)); r2 = side.arr(np.zeros(nx))
        a = (C.c_double * nx)(*alpha)
        L = side.lib
        assert L.hipk_axpy_cols(side.ctx, dt, m, a, side.ptr(x), ld, side.ptr(y), ld, nx) == 0
        assert L.hipk_scale_cols(side.ctx, dt, m, side.ptr(x), ld, nx, a) == 0
        assert L.hipk_gather_cols(side.ctx, dt, m, side.ptr(y), ld, perm.ctypes.data_as(C.POINTER(C.c_int)), nx, side.ptr(z), ld) == 0
        assert L.hipk_col_norms2(side.ctx, dt, m, side.ptr(z), ld, nx, side.ptr(n2)) == 0
        assert L.hipk_residual_cols(side.ctx, dt, m, side.ptr(x), ld, side.ptr(z), ld, nx, a, side.ptr(r2)) == 0
        assert L.hipk_copy_cols(side.ctx, dt, m, side.ptr(z), ld, side.ptr(y), ld, 2) == 0
        res.append([side.get(t) for t in (x, y, z, n2, r2)])
        side.close()
    tol = 1e-13 if dt == F.HIPK_F64 else 1e-5
    for a_, b_ in zip(res[0][:3], res[1][:3]):
        assert np.max(np.abs(a_[:, :m] - b_[:, :m])) <= tol * 10
    assert np.allclose(res[0][3], res[1][3], rtol=tol * 100)
    assert np.allclose(res[0][4], res[1][4], rtol=tol * 100)


@pytest.mark.parametrize("dt", [F.HIPK_F64, F.HIPK_F32])
@pytest.mark.parametrize("m,nx", [(777, 1), (123457, 3), (300001, 8)])
def test_qmr_recurrence_kernels(built, dt, m, nx):
    """hipk_pair_dots / hipk_qmr_update (block QMR of the JDQMR inner solver)."""
    rng = np.random.default_rng(13 * m + nx)
    npdt = NPDT[dt]
    ld = m + 3
    X, Y, D, Dl, S = (rng.standard_normal((nx, ld)).astype(npdt) for _ in range(5))
    gam, eta = rng.standard_normal(nx), rng.standard_normal(nx)
    res = []
    for side in (Dev(), Host()):
        x, y, d, dl, so = (side.arr(t) for t in (X, Y, D, Dl, S))
        o1 = side.arr(np.zeros(nx)); o2 = side.arr(np.zeros(nx))
        L = side.lib
        assert L.hipk_pair_dots(side.ctx, dt, m, side.ptr(x), ld, side.ptr(y), ld, nx, side.ptr(o1)) == 0
        assert L.hipk_qmr_update(side.ctx, dt, m, nx, (C.c_double * nx)(*gam), (C.c_double * nx)(*eta), side.ptr(d), ld,
                                 side.ptr(dl), ld, side.ptr(so), ld, side.ptr(o2)) == 0
        # fused axpy + dot (z'y and y'y flavours) and y = a y + x
        o3 = side.arr(np.zeros(nx)); o4 = side.arr(np.zeros(nx))
        assert L.hipk_axpy_dot(side.ctx, dt, m, nx, (C.c_double * nx)(*gam), side.ptr(x), ld, side.ptr(y), ld,
                               side.ptr(d), ld, side.ptr(o3)) == 0
        assert L.hipk_axpy_dot(side.ctx, dt, m, nx, (C.c_double * nx)(*eta), side.ptr(d), ld, side.ptr(y), ld,
                               None, 0, side.ptr(o4)) == 0
        assert L.hipk_xpay_cols(side.ctx, dt, m, (C.c_double * nx)(*gam), side.ptr(y), ld, side.ptr(x), ld, nx) == 0
        res.append([side.get(t) for t in (o1, o2, dl, so, o3, o4, y, x)])
        side.close()
    tol = 1e-12 if dt == F.HIPK_F64 else 2e-5
    Xd, Yd, Dd = (t[:, :m].astype(np.float64) for t in (X, Y, D))
    y1 = (Yd + gam[:, None] * Xd).astype(npdt).astype(np.float64)
    assert np.max(np.abs(res[1][4] - np.einsum("ij,ij->i", Dd, y1))) <= tol * np.sqrt(m) * 16
    for q in (4, 5):
        assert np.max(np.abs(res[0][q] - res[1][q])) <= tol * np.sqrt(m) * 16 * max(1.0, np.abs(res[1][q]).max() / m)
    for q in (6, 7):
        assert np.max(np.abs(res[0][q][:, :m] - res[1][q][:, :m])) <= (1e-13 if dt == F.HIPK_F64 else 1e-5) * 50
        assert np.array_equal(res[0][q][:, m:], res[1][q][:, m:])
    ref_dots = np.einsum("ij,ij->i", X[:, :m].astype(np.float64), Y[:, :m].astype(np.float64))
    assert np.max(np.abs(res[0][0] - res[1][0])) <= tol * np.sqrt(m) * 4
    assert np.max(np.abs(res[1][0] - ref_dots)) <= tol * np.sqrt(m) * 4
    assert np.allclose(res[0][1], res[1][1], rtol=tol * 100)
    for a_, b_ in zip(res[0][2:4], res[1][2:4]):
        assert np.max(np.abs(a_[:, :m] - b_[:, :m])) <= (1e-13 if dt == F.HIPK_F64 else 1e-5) * 10
        assert np.array_equal(a_[:, m:], b_[:, m:])      # padding rows untouched


@pytest.mark.parametrize("dt", [F.HIPK_F64, F.HIPK_F32])
@pytest.mark.parametrize("ncols", [1, 3, 8])
def test_csr_matvec(built, dt, ncols):
    npdt = NPDT[dt]
    for name, rp, ci, va, n in _csr_cases():
        rng = np.random.default_rng(n)
        ld = n + 2
        X = rng.standard_normal((ncols, ld)).astype(npdt)
        res = []
        for side in (Dev(), Host()):
            A = C.c_void_p()
            vv = np.ascontiguousarray(va, dtype=npdt)
            assert side.lib.hipk_csr_create(side.ctx, dt, n, n, 0, rp.ctypes.data_as(C.c_void_p),
                                            ci.ctypes.data_as(C.c_void_p), vv.ctypes.data_as(C.c_void_p), C.byref(A)) == 0
            x = side.arr(X); y = side.arr(np.zeros_like(X))
            assert side.lib.hipk_csr_matvec(A, None, side.ptr(x), ld, side.ptr(y), ld, ncols) == 0
            res.append(side.get(y)[:, :n])
            side.lib.hipk_csr_destroy(A)
            side.close()
        ref = problems.csr_matvec_numpy(rp, ci, va.astype(npdt).astype(np.float64), X[:, :n].T.astype(np.float64)).T
        tol = 1e-12 if dt == F.HIPK_F64 else 2e-4
        assert np.max(np.abs(res[0] - res[1])) <= tol * (1 + np.abs(res[1]).max()), name
        assert np.max(np.abs(res[1] - ref)) <= tol * (1 + np.abs(ref).max()), name


@pytest.mark.parametrize("dt", [F.HIPK_F64, F.HIPK_F32])
def test_csr_queries_across_format_switch(built, dt):
    """The queries about the form in use all read the one routing decision: for the banded matrix (row tiles with the 2-byte
    index stream; no other form is built for it) format, index bytes and the bytes of the plain and the fused one-column
    product have their closed forms, and a hipk_set_spmv_format(0 / 1) round trip leaves them as they were."""
    name, rp, ci, va, n = [c for c in _csr_cases() if c[0] == "banded"][0]
    npdt = NPDT[dt]
    es, nnz = np.dtype(npdt).itemsize, len(ci)
    side = Dev()
    lib = side.lib
    lib.hipk_set_spmv_format.argtypes = [C.c_int]
    lib.hipk_csr_format.argtypes = [C.c_void_p]; lib.hipk_csr_index_bytes.argtypes = [C.c_void_p]
    lib.hipk_csr_product_bytes.argtypes = [C.c_void_p, C.c_int]; lib.hipk_csr_product_bytes.restype = C.c_double
    A = C.c_void_p()
    vv = np.ascontiguousarray(va, dtype=npdt)
    assert lib.hipk_csr_create(side.ctx, dt, n, n, 0, rp.ctypes.data_as(C.c_void_p), ci.ctypes.data_as(C.c_void_p),
                               vv.ctypes.data_as(C.c_void_p), C.byref(A)) == 0
    read = lambda: (lib.hipk_csr_format(A), lib.hipk_csr_index_bytes(A), lib.hipk_csr_product_bytes(A, 0), lib.hipk_csr_product_bytes(A, 1))
    want = (0, 2, nnz * (es + 2) + (n + 1) * 4.0 + 2.0 * n * es, nnz * (es + 2) + (n + 1) * 4.0 + 3.0 * n * es)
    old = lib.hipk_set_spmv_format(1)
    try:
        seen = [read()]
        for fmt in (0, 1):
            lib.hipk_set_spmv_format(fmt)
            seen.append(read())
    finally:
        lib.hipk_set_spmv_format(old)
        lib.hipk_csr_destroy(A)
        side.close()
    assert seen == [want] * 3, seen


def test_inkernel_second_stage_agrees_with_separate_launches(built):
    """The alternative second stage of the three reductions of a block-size-1 iteration (csrc/hipk_internal.h:
    two-level, inside the producing launch, write-through partial sums; off by default because it is slower): same
    sums as the separate launches up to the summation order, bit-reproducible from launch to launch (40 launches of the
    fused residual pass under load), and a whole solve through it converges to the same pairs."""
    lib = F.load_product()
    lib.hipk_set_inkernel_fin.argtypes = [C.c_int]
    m, k, L = 400_003, 14, 6
    rng = np.random.default_rng(5)
    ld = m + 3
    V = rng.standard_normal((k + 1, ld)); W = rng.standard_normal((k + 1, ld)); Q = rng.standard_normal((L, ld))
    h = np.ascontiguousarray(rng.standard_normal(k) / np.sqrt(k))
    outs = {}
    old = lib.hipk_set_inkernel_fin(0)
    try:
        for mask in (0, 7):
            lib.hipk_set_inkernel_fin(mask)
            side = Dev()
            v, w, q = side.arr(V), side.arr(W), side.arr(Q)
            out = side.arr(np.zeros(2 * (k + L) + 1))
            seen = []
            for rep in range(40):
                assert side.lib.hipk_ritz_residual_overlaps(side.ctx, F.HIPK_F64, m, side.ptr(v), side.ptr(w), ld, k, h.ctypes.data_as(C.c_void_p),
                                                            C.c_double(0.37), side.ptr(v, k * ld), side.ptr(q), ld, L, 1, side.ptr(out)) == 0
                seen.append(side.get(out).copy())
            for s_ in seen[1:]:
                assert np.array_equal(s_, seen[0]), mask          # reproducible bits
            outs[mask] = seen[0]
            side.close()
        scale = np.sqrt(m) * 4
        assert np.max(np.abs(outs[0] - outs[7])) <= 1e-12 * scale * max(1.0, np.abs(outs[0]).max() / scale)
        # a whole solve through the in-kernel form
        dims = (40, 41, 42)
        rp, ci, va, n = problems.laplacian_csr(dims)
        kw = dict(numEvals=6, method="GD_plusK", eps=1e-9, aNorm=12.0, v0=problems.start_vector(n))
        lib.hipk_set_inkernel_fin(0)
        a = checkers.eigsh(checkers.Operator(n, csr=(rp, ci, va)), backend="hip", **kw)
        lib.hipk_set_inkernel_fin(7)
        b = checkers.eigsh(checkers.Operator(n, csr=(rp, ci, va)), backend="hip", **kw)
        assert a.ret == 0 and b.ret == 0
        assert np.max(np.abs(a.evals - b.evals)) <= 1e-11 * 12.0
        assert abs(a.stats["numOuterIterations"] - b.stats["numOuterIterations"]) <= max(2, 0.02 * a.stats["numOuterIterations"])
    finally:
        lib.hipk_set_inkernel_fin(old)


@pytest.mark.parametrize("dt", [F.HIPK_F64, F.HIPK_F32])
def test_csr_panel_blocked_scattered_pattern(built, dt):
    """BASELINE configs[4]'s pattern in small (5 entries per row at (i p_q + q) mod n) and its transpose: the input
    vector is larger than an XCD's L2 and consecutive rows share no cache line, so hipk_csr_create_rect also builds the
    panel-blocked form (csrc/hipk_sparse_pb.hip) and one- and two-column products go through it; wider blocks through
    the plain CSR kernels.  Against the plain-C restatement and numpy; twice, bit for bit the same."""
    from primme_amd.svds_api import transpose_csr
    npdt = NPDT[dt]
    m, n = (800_000, 900_000) if dt == F.HIPK_F64 else (1_700_000, 1_600_000)    # both vectors above the 6 MB threshold
    rp, ci, va = problems.svds_synthetic_csr(m, n)
    rpT, ciT, vaT = transpose_csr(m, n, rp, ci, va)
    for name, (mm, nn, r_, c_, v_) in {"A": (m, n, rp, ci, va), "At": (n, m, rpT, ciT, vaT)}.items():
        rng = np.random.default_rng(mm % 1000)
        for ncols in (1, 2, 3):
            X = rng.standard_normal((ncols, nn)).astype(npdt)
            res = []
            for side in (Dev(), Host()):
                A = C.c_void_p()
                vv = np.ascontiguousarray(v_, dtype=npdt)
                assert side.lib.hipk_csr_create_rect(side.ctx, dt, mm, nn, r_.ctypes.data_as(C.c_void_p), c_.ctypes.data_as(C.c_void_p),
                                                     vv.ctypes.data_as(C.c_void_p), C.byref(A)) == 0
                if side.name == "hip":
                    side.lib.hipk_csr_panels.argtypes = [C.c_void_p]
                    assert side.lib.hipk_csr_panels(A) >= 2, name          # the panel-blocked form was built
                x = side.arr(X); y = side.arr(np.zeros((ncols, mm), dtype=npdt))
                assert side.lib.hipk_csr_matvec(A, None, side.ptr(x), nn, side.ptr(y), mm, ncols) == 0
                first = side.get(y).copy()
                assert side.lib.hipk_csr_matvec(A, None, side.ptr(x), nn, side.ptr(y), mm, ncols) == 0
                assert np.array_equal(first, side.get(y)), name            # reproducible bits
                res.append(first)
                side.lib.hipk_csr_destroy(A)
                side.close()
            ref = problems.csr_matvec_numpy(r_, c_, np.asarray(v_).astype(npdt).astype(np.float64), X.T.astype(np.float64)).T
            tol = 1e-12 if dt == F.HIPK_F64 else 2e-4
            assert np.max(np.abs(res[0] - res[1])) <= tol * (1 + np.abs(res[1]).max()), (name, ncols)
            assert np.max(np.abs(res[0] - ref)) <= tol * (1 + np.abs(ref).max()), (name, ncols)


@pytest.mark.parametrize("dt", [F.HIPK_F64, F.HIPK_F32])
@pytest.mark.parametrize("ncols", [2, 8])
def test_csr_matvec_shifted(built, dt, ncols):
    """y = A x - shift[c] x(:,c) in one launch (the first update of the projected operator of the JDQMR inner
    iteration fused into the SpMM), windowed and gather tiles alike"""
    npdt = NPDT[dt]
    for name, rp, ci, va, n in _csr_cases():
        rng = np.random.default_rng(n + ncols)
        ld = n + 2
        X = rng.standard_normal((ncols, ld)).astype(npdt)
        shifts = rng.standard_normal(ncols) * 3
        res = []
        for side in (Dev(), Host()):
            A = C.c_void_p()
            vv = np.ascontiguousarray(va, dtype=npdt)
            assert side.lib.hipk_csr_create(side.ctx, dt, n, n, 0, rp.ctypes.data_as(C.c_void_p),
                                            ci.ctypes.data_as(C.c_void_p), vv.ctypes.data_as(C.c_void_p), C.byref(A)) == 0
            x = side.arr(X); y = side.arr(np.zeros_like(X))
            sh = (C.c_double * ncols)(*shifts)
            assert side.lib.hipk_csr_matvec_shifted(A, None, side.ptr(x), ld, side.ptr(y), ld, ncols, sh) == 0
            res.append(side.get(y)[:, :n])
            side.lib.hipk_csr_destroy(A)
            side.close()
        ref = problems.csr_matvec_numpy(rp, ci, va.astype(npdt).astype(np.float64), X[:, :n].T.astype(np.float64)).T - shifts[:, None] * X[:, :n]
        tol = 1e-12 if dt == F.HIPK_F64 else 2e-4
        assert np.max(np.abs(res[0] - res[1])) <= tol * (1 + np.abs(res[1]).max()), name
        assert np.max(np.abs(res[1] - ref)) <= tol * (1 + np.abs(ref).max()), name


@pytest.mark.parametrize("dt", [F.HIPK_F64, F.HIPK_F32])
@pytest.mark.parametrize("nx,L", [(8, 19), (5, 3), (2, 9), (1, 1), (8, 40)])
def test_project_and_triple_dots_in_one_pass(built, dt, nx, L):
    """hipk_project_triple_dots (round 6): W -= Q c and [x'w | v'w | v'x] of the updated W in one pass — the projection of
    (A - shift) d against the locked vectors and the three inner products of a block QMR step.  Must be the pair of launches
    it replaces BIT FOR BIT on the device (same fma order per element, same partial sums): the history of a JDQMR solve does
    not move; and agree with the plain-C restatement and numpy."""
    rng = np.random.default_rng(100 * nx + L)
    npdt = NPDT[dt]
    m, ld = 90001, 90004
    Q = rng.standard_normal((L, ld)).astype(npdt); X, Vv, W = (rng.standard_normal((nx, ld)).astype(npdt) for _ in range(3))
    coef = rng.standard_normal((nx, L + 3))          # ldcoef = L + 3
    res = {}
    for side in (Dev(), Host()):
        q, x, v = side.arr(Q), side.arr(X), side.arr(Vv)
        segs = segs_array(side, [(q, 0, ld, L)])
        for mode in ("fused", "pair"):
            w = side.arr(W); cf = side.arr(coef); o3 = side.arr(np.zeros(3 * nx))
            if mode == "fused":
                assert side.lib.hipk_project_triple_dots(side.ctx, dt, m, segs, 1, side.ptr(cf), L + 3, side.ptr(w), ld, nx, side.ptr(x), ld, side.ptr(v), ld, side.ptr(o3)) == 0
            else:
                assert side.lib.hipk_panel_project(side.ctx, dt, m, segs, 1, side.ptr(cf), L + 3, side.ptr(w), ld, nx, None) == 0
                assert side.lib.hipk_triple_dots(side.ctx, dt, m, side.ptr(x), ld, side.ptr(v), ld, side.ptr(w), ld, nx, side.ptr(o3)) == 0
            res[(side.name, mode)] = (side.get(w)[:, :m].copy(), side.get(o3).copy())
        side.close()
    assert np.array_equal(res[("hip", "fused")][0], res[("hip", "pair")][0])
    assert np.array_equal(res[("hip", "fused")][1], res[("hip", "pair")][1])
    Wref = W[:, :m].astype(np.float64) - coef[:, :L] @ Q[:, :m].astype(np.float64)
    X64, V64 = X[:, :m].astype(np.float64), Vv[:, :m].astype(np.float64)
    ref3 = np.concatenate([np.sum(X64 * Wref, axis=1), np.sum(V64 * Wref, axis=1), np.sum(V64 * X64, axis=1)])
    tol = 1e-12 if dt == F.HIPK_F64 else 3e-4
    for key, (wg, d3) in res.items():
        assert np.max(np.abs(wg - Wref)) <= tol * (1 + np.abs(Wref).max()) * max(1, L) ** 0.5, key
        assert np.max(np.abs(d3 - ref3)) <= tol * np.sqrt(m) * 4 * max(1, L) ** 0.5, key


@pytest.mark.parametrize("dt", [F.HIPK_F64, F.HIPK_F32])
def test_qmr_projection_folded_into_residual_update(built, dt):
    """sigma = v'(I - x x')w from one pass of three inner products, then g -= alpha (w - (x'w) x), |g|^2 in one pass:
    equal to projecting w first and updating g afterwards (the two passes and the extra synchronisation it replaces)"""
    rng = np.random.default_rng(33)
    npdt = NPDT[dt]
    m, ld, nx = 80003, 80004, 6
    X, Vv, W, G = (rng.standard_normal((nx, ld)).astype(npdt) for _ in range(4))
    alpha = rng.standard_normal(nx)
    res = []
    for side in (Dev(), Host()):
        x, v, w, g = side.arr(X), side.arr(Vv), side.arr(W), side.arr(G)
        o3 = side.arr(np.zeros(3 * nx)); o1 = side.arr(np.zeros(nx))
        assert side.lib.hipk_triple_dots(side.ctx, dt, m, side.ptr(x), ld, side.ptr(v), ld, side.ptr(w), ld, nx, side.ptr(o3)) == 0
        d3 = side.get(o3).copy()
        a = (C.c_double * nx)(*alpha); xr = (C.c_double * nx)(*d3[:nx])
        assert side.lib.hipk_axpy_proj_dot(side.ctx, dt, m, nx, a, xr, side.ptr(w), ld, side.ptr(x), ld, side.ptr(g), ld, side.ptr(o1)) == 0
        res.append((d3, side.get(g)[:, :m], side.get(o1)))
        side.close()
    X64, V64, W64, G64 = (t[:, :m].astype(np.float64) for t in (X, Vv, W, G))
    tol = 1e-12 if dt == F.HIPK_F64 else 2e-4
    ref3 = np.concatenate([np.sum(X64 * W64, axis=1), np.sum(V64 * W64, axis=1), np.sum(V64 * X64, axis=1)])
    for r in res:
        assert np.max(np.abs(r[0] - ref3)) <= tol * np.sqrt(m) * 4
    xr = res[1][0][:nx]
    gref = G64 - alpha[:, None] * (W64 - xr[:, None] * X64)
    assert np.max(np.abs(res[1][1] - gref)) <= tol * 20 and np.max(np.abs(res[0][1] - res[1][1])) <= tol * 20
    assert np.max(np.abs(res[0][2] - res[1][2]) / (1 + res[1][2])) <= tol * np.sqrt(m)


@pytest.mark.parametrize("dt", [F.HIPK_F64, F.HIPK_F32])
def test_qmr_update_with_jacobi(built, dt):
    """delta = gamma delta + eta d; sol += delta; |sol|^2 and w = g ./ (diag - shift), g'w in one pass"""
    rng = np.random.default_rng(21)
    npdt = NPDT[dt]
    m, ld, nx = 90001, 90004, 5
    D, De, So, G = (rng.standard_normal((nx, ld)).astype(npdt) for _ in range(4))
    diag = (2.0 + rng.random(m)).astype(npdt); diag[7] = 1.0     # shift 1.0 makes this denominator zero -> clamped
    gam, eta, sh = rng.standard_normal(nx), rng.standard_normal(nx), np.array([1.0, 0.3, -2.0, 0.0, 1.5])
    res = []
    for side in (Dev(), Host()):
        d, de, so, g = side.arr(D), side.arr(De), side.arr(So), side.arr(G)
        dg = side.arr(diag); w = side.arr(np.zeros((nx, ld), dtype=npdt)); out = side.arr(np.zeros(2 * nx))
        a = lambda v: (C.c_double * nx)(*v)
        assert side.lib.hipk_qmr_update_jacobi(side.ctx, dt, m, nx, a(gam), a(eta), side.ptr(d), ld, side.ptr(de), ld, side.ptr(so), ld,
                                               side.ptr(g), ld, side.ptr(dg), a(sh), C.c_double(1e-10), side.ptr(w), ld, side.ptr(out)) == 0
        res.append([side.get(t) for t in (de, so, w, out)])
        side.close()
    tol = 1e-12 if dt == F.HIPK_F64 else 2e-4
    de_ref = De[:, :m].astype(np.float64) * gam[:, None] + D[:, :m].astype(np.float64) * eta[:, None]
    den = diag.astype(np.float64)[None, :] - sh[:, None]
    den = np.where(np.abs(den) > 1e-10, den, np.copysign(1e-10, den))
    w_ref = G[:, :m].astype(np.float64) / den
    for a_, b_ in zip(res[0][:3], res[1][:3]):
        assert np.max(np.abs(a_[:, :m] - b_[:, :m]) / (1 + np.abs(b_[:, :m]))) <= tol * 10
    assert np.max(np.abs(res[1][0][:, :m] - de_ref)) <= tol * 10 * (1 + np.abs(de_ref).max())
    assert np.max(np.abs(res[1][2][:, :m] - w_ref) / (1 + np.abs(w_ref))) <= tol * 10
    assert np.max(np.abs(res[0][3] - res[1][3]) / (1 + np.abs(res[1][3]))) <= tol * np.sqrt(m)


@pytest.mark.parametrize("dt", [F.HIPK_F64, F.HIPK_F32])
@pytest.mark.parametrize("nx", [3, 8, 11])
def test_qmr_early_rho_pair(built, dt, nx):
    """The two passes of a block QMR step with the next rho taken early: g -= alpha (w - xr x), |g|^2 and g'K^-1 g in
    one pass; delta / sol update and the new direction d = K^-1 g + beta d in place in the next.  Against the oracle and
    against the sequence they replace (axpy_proj_dot, qmr_update_jacobi, w += beta d): same arithmetic per element."""
    rng = np.random.default_rng(77 + nx)
    npdt = NPDT[dt]
    m, ld = 70003, 70004
    X, W, G, D, De, So = (rng.standard_normal((nx, ld)).astype(npdt) for _ in range(6))
    diag = (2.0 + rng.random(m)).astype(npdt); diag[5] = 1.0
    alpha, xr, gam, eta, beta = (rng.standard_normal(nx) for _ in range(5))
    sh = np.resize(np.array([1.0, 0.3, -2.0, 0.0, 1.5]), nx)
    a = lambda v: (C.c_double * nx)(*v)
    res = []
    for side in (Dev(), Host()):
        x, w, g, d, de, so, dg = (side.arr(t) for t in (X, W, G, D, De, So, diag))
        o2, o1 = side.arr(np.zeros(2 * nx)), side.arr(np.zeros(nx))
        assert side.lib.hipk_axpy_proj_dot_jacobi(side.ctx, dt, m, nx, a(alpha), a(xr), side.ptr(w), ld, side.ptr(x), ld, side.ptr(g), ld,
                                                  side.ptr(dg), a(sh), C.c_double(1e-10), side.ptr(o2)) == 0
        assert side.lib.hipk_qmr_update_dir(side.ctx, dt, m, nx, a(gam), a(eta), a(beta), side.ptr(d), ld, side.ptr(de), ld, side.ptr(so), ld,
                                            side.ptr(g), ld, side.ptr(dg), a(sh), C.c_double(1e-10), side.ptr(o1)) == 0
        new = [side.get(t).copy() for t in (g, d, de, so, o2, o1)]
        # the replaced sequence on fresh copies
        g2, d2, de2, so2 = (side.arr(t) for t in (G, D, De, So))
        w2 = side.arr(np.zeros((nx, ld), dtype=npdt)); p1, p2 = side.arr(np.zeros(nx)), side.arr(np.zeros(2 * nx))
        assert side.lib.hipk_axpy_proj_dot(side.ctx, dt, m, nx, a(alpha), a(xr), side.ptr(w), ld, side.ptr(x), ld, side.ptr(g2), ld, side.ptr(p1)) == 0
        assert side.lib.hipk_qmr_update_jacobi(side.ctx, dt, m, nx, a(gam), a(eta), side.ptr(d2), ld, side.ptr(de2), ld, side.ptr(so2), ld,
                                               side.ptr(g2), ld, side.ptr(dg), a(sh), C.c_double(1e-10), side.ptr(w2), ld, side.ptr(p2)) == 0
        assert side.lib.hipk_axpy_cols(side.ctx, dt, m, a(beta), side.ptr(d2), ld, side.ptr(w2), ld, nx) == 0
        old = [side.get(t).copy() for t in (g2, w2, de2, so2)] + [np.concatenate([side.get(p1), side.get(p2)[nx:]]), side.get(p2)[:nx].copy()]
        res.append((new, old))
        side.close()
    tol = 1e-12 if dt == F.HIPK_F64 else 2e-4
    for new, old in res:                                  # new sequence == old sequence, element for element
        for t in range(4):
            assert np.array_equal(new[t][:, :m], old[t][:, :m]), t
        for t in (4, 5):
            assert np.max(np.abs(new[t] - old[t]) / (1 + np.abs(old[t]))) <= tol * np.sqrt(m)
    for t in range(4):                                    # device == oracle
        assert np.max(np.abs(res[0][0][t][:, :m] - res[1][0][t][:, :m]) / (1 + np.abs(res[1][0][t][:, :m]))) <= tol * 10
    for t in (4, 5):
        assert np.max(np.abs(res[0][0][t] - res[1][0][t]) / (1 + np.abs(res[1][0][t]))) <= tol * np.sqrt(m)
    for t in range(4):                                    # padding untouched
        assert np.array_equal(res[0][0][t][:, m:], (G, D, De, So)[t][:, m:])


@pytest.mark.parametrize("dt", [F.HIPK_F64, F.HIPK_F32])
def test_csr_matvec_scaled_fused_tail(built, dt):
    """y = A (a x), xout = a x, dot = xout' y with a = 1/sqrt(norm2) read from device memory: one launch for the
    normalisation, the operator and t'At of the one-synchronisation iteration; against the oracle and against
    the separate launches it replaces (same arithmetic per element)."""
    npdt = NPDT[dt]
    for name, rp, ci, va, n in _csr_cases():
        rng = np.random.default_rng(n + 5)
        X = rng.standard_normal(n).astype(npdt) * 3.0
        n2 = np.array([float(np.sum(X.astype(np.float64) ** 2))])
        res = []
        for side in (Dev(), Host()):
            A = C.c_void_p()
            vv = np.ascontiguousarray(va, dtype=npdt)
            assert side.lib.hipk_csr_create(side.ctx, dt, n, n, 0, rp.ctypes.data_as(C.c_void_p),
                                            ci.ctypes.data_as(C.c_void_p), vv.ctypes.data_as(C.c_void_p), C.byref(A)) == 0
            x = side.arr(X); xo = side.arr(np.zeros_like(X)); y = side.arr(np.zeros_like(X))
            nn = side.arr(n2); dot = side.arr(np.zeros(1))
            assert side.lib.hipk_csr_matvec_scaled(A, side.ctx, side.ptr(x), side.ptr(nn), side.ptr(xo), side.ptr(y), side.ptr(dot)) == 0
            # the launches it replaces
            x2 = side.arr(X); y2 = side.arr(np.zeros_like(X))
            assert side.lib.hipk_scale_cols_rsqrt_dev(side.ctx, dt, n, side.ptr(x2), n, 1, side.ptr(nn)) == 0
            assert side.lib.hipk_csr_matvec(A, None, side.ptr(x2), n, side.ptr(y2), n, 1) == 0
            res.append([side.get(t) for t in (xo, y, dot, x2, y2)])
            side.lib.hipk_csr_destroy(A)
            side.close()
        tol = 1e-12 if dt == F.HIPK_F64 else 2e-4
        for a_, b_ in zip(res[0][:2], res[1][:2]):
            assert np.max(np.abs(a_ - b_)) <= tol * (1 + np.abs(b_).max()), name
        assert abs(res[0][2][0] - res[1][2][0]) <= tol * np.sqrt(n) * (1 + abs(res[1][2][0])), name
        assert np.array_equal(res[0][0], res[0][3]), name          # normalised vector: bit-identical to the scale kernel
        assert np.max(np.abs(res[0][1] - res[0][4])) <= tol * (1 + np.abs(res[0][4]).max()), name
        assert abs(res[0][2][0] - float(res[0][0].astype(np.float64) @ res[0][1].astype(np.float64))) <= tol * np.sqrt(n) * (1 + abs(res[0][2][0])), name


def _rr_arrow_case(side, k, L, cand, largest, grow_row, seed):
    """hipk_rr_arrow against numpy: the pair the kernel returns must be the cand-th eigenpair of the arrowhead matrix its
    inputs define, mapped back to the basis [V t]; then the residual pass that reads the pair from device memory
    (hipk_ritz_residual_overlaps_dev) must equal the one that gets it by value."""
    rng = np.random.default_rng(seed)
    Hk = rng.standard_normal((k, k)); Hk = (Hk + Hk.T) / 2 + np.diag(np.linspace(-2.0, 3.0, k))
    th, Y = np.linalg.eigh(Hk)
    if largest:
        th, Y = th[::-1].copy(), Y[:, ::-1].copy()
    G = rng.standard_normal((k, L)) * 0.1
    cV, cQ, wr, grow = rng.standard_normal(k) * 1e-3, rng.standard_normal(L) * 0.1, rng.standard_normal(k), rng.standard_normal(L) * 0.1
    n2, alpha = 0.7 + rng.random(), float(rng.standard_normal())
    nfov = 2 * (k + L) + 1
    fov = np.concatenate([cV, cQ, [0.3], wr, grow, [n2]])
    Guse = G.copy()
    if grow_row and L > 0:
        Guse[k - 1] = grow
    hc = (wr - Y @ (th * (Y.T @ cV)) - Guse @ cQ) / np.sqrt(n2)
    z = Y.T @ hc
    M = np.zeros((k + 1, k + 1)); M[:k, :k] = np.diag(th); M[:k, k] = z; M[k, :k] = z; M[k, k] = alpha
    w, U = np.linalg.eigh(M)
    idx = (k - cand) if largest else cand
    lam, y = w[idx], U[:, idx]
    hwant = np.concatenate([Y @ y[:k], [y[k]]])
    inp = F.HipkRrIn()
    inp.k, inp.L, inp.cand, inp.largest, inp.grow_row = k, L, cand, int(largest), int(grow_row)
    for i in range(k):
        inp.theta[i] = th[i]
        for r in range(k):
            inp.Y[r + i * k] = Y[r, i]
    for l in range(L):
        for j in range(k):
            inp.G[j + l * k] = G[j, l]
    fd, ad, out = side.arr(fov), side.arr(np.array([alpha])), side.arr(np.zeros(64))
    assert side.lib.hipk_rr_arrow(side.ctx, C.byref(inp), side.ptr(fd), nfov, side.ptr(ad), side.ptr(out)) == 0
    got = side.get(out)
    assert got[33] == 0.0, (k, L, cand, largest, got[33])
    scale = max(1.0, np.abs(w).max())
    assert abs(got[32] - lam) <= 1e-13 * scale, (k, cand, got[32], lam)
    h = got[:k + 1]
    gaps = np.abs(w - lam); gaps[idx] = np.inf
    tol = 1e-13 * scale / min(1.0, gaps.min())            # an eigenvector is determined to eps |M| / gap
    assert min(np.max(np.abs(h - hwant)), np.max(np.abs(h + hwant))) <= 10 * tol, (k, L, cand, largest)
    Hfull = np.zeros((k + 1, k + 1)); Hfull[:k, :k] = Y @ np.diag(th) @ Y.T; Hfull[:k, k] = hc; Hfull[k, :k] = hc; Hfull[k, k] = alpha
    assert np.max(np.abs(Hfull @ h - got[32] * h)) <= 2e-13 * scale and abs(h @ h - 1.0) <= 1e-13
    return out, h, got[32]


@pytest.mark.parametrize("largest", [0, 1])
def test_rr_arrow_pair_of_the_next_iteration(built, largest):
    """The one-wave Rayleigh-Ritz kernel of the iteration that is enqueued before the host has seen the previous one
    (include/primme_amd_kernels.h: hipk_rr_arrow): every root index, both targets, with and without locked vectors, and the
    residual pass that takes its pair from device memory."""
    for side in (Dev(), Host()):
        seed = 0
        for k, L in ((1, 0), (2, 0), (5, 3), (9, 0), (15, 10), (16, 4)):
            for cand in sorted({0, 1, k // 2, k - 1, k} & set(range(k + 1))):
                seed += 1
                out, h, lam = _rr_arrow_case(side, k, L, cand, largest, grow_row=(L > 0 and cand % 2 == 0), seed=seed)
        # the residual pass reading (h, theta) from device memory == the one that gets them by value
        k, L, m = 15, 10, 70001
        out, h, lam = _rr_arrow_case(side, k, L, 0, largest, True, 99)
        rng = np.random.default_rng(5)
        ld = m + 1
        V = rng.standard_normal((k + 1, ld)); W = rng.standard_normal((k + 1, ld)); Q = rng.standard_normal((L, ld))
        v, w, q = side.arr(V), side.arr(W), side.arr(Q)
        res = []
        for dev in (0, 1):
            dst = side.arr(np.zeros((1, ld))); o = side.arr(np.zeros(4 * (k + 1 + L) + 4))
            if dev:
                assert side.lib.hipk_ritz_residual_overlaps_dev(side.ctx, F.HIPK_F64, m, side.ptr(v), side.ptr(w), ld, k + 1, side.ptr(out), side.ptr(dst),
                                                                side.ptr(q), ld, L, 1, side.ptr(o)) == 0
            else:
                hh = np.zeros(32); hh[:k + 1] = h
                assert side.lib.hipk_ritz_residual_overlaps(side.ctx, F.HIPK_F64, m, side.ptr(v), side.ptr(w), ld, k + 1, hh.ctypes.data_as(C.c_void_p),
                                                            C.c_double(lam), side.ptr(dst), side.ptr(q), ld, L, 1, side.ptr(o)) == 0
            res.append((side.get(dst), side.get(o)))
        assert np.array_equal(res[0][0], res[1][0]) and np.array_equal(res[0][1], res[1][1])
        side.close()


@pytest.mark.parametrize("dt", [F.HIPK_F64, F.HIPK_F32])
@pytest.mark.parametrize("case", ["lap3d", "lap2d", "random"])
def test_tail_without_second_stage_launches(built, dt, case):
    """Round 6 (include/primme_amd_kernels.h: hipk_tail_defer / hipk_tail_finish): the tail of a block-size-1 iteration —
    Gram-Schmidt update + |t|^2, then scale + A t + t'At — with ONE small launch at its end instead of two second-stage
    launches and the one-wave Rayleigh-Ritz launch.  Checked against the sequence of separate launches on the same data:
    the published |t|^2 is EXACTLY the number the operator launch scaled with (the normalised vector is a x with
    a = 1 / sqrt(|t|^2) of the published value, bit for bit), t'At is the sum over the vectors actually written, both agree
    with the separate sequence to rounding, the Rayleigh-Ritz step inside the launch returns the bits of hipk_rr_arrow on the
    same reductions; the row-pattern operator takes both deferrals, the tile kernel only that of t'At."""
    npdt = NPDT[dt]
    rng = np.random.default_rng(21)
    if case == "lap3d": rp, ci, va, n = problems.laplacian_csr((61, 62, 63))
    elif case == "lap2d": rp, ci, va, n = problems.laplacian_csr((700, 701))
    else:
        n = 300_007
        counts = rng.integers(1, 9, size=n)
        rp = np.zeros(n + 1, dtype=np.int64); np.cumsum(counts, out=rp[1:]); rp = rp.astype(np.int32)
        ci = np.concatenate([np.sort(rng.choice(np.arange(max(0, i - 40), min(n, i + 40)), size=c, replace=False)) for i, c in enumerate(counts)]).astype(np.int32)
        va = rng.standard_normal(len(ci))
    k, L = 9, 4
    side = Dev()
    lib = side.lib
    lib.hipk_csr_format.argtypes = [C.c_void_p]
    lib.hipk_tail_abandon.argtypes = [C.c_void_p]; lib.hipk_tail_abandon.restype = None
    A = C.c_void_p()
    vv = np.ascontiguousarray(va, dtype=npdt)
    assert lib.hipk_csr_create(side.ctx, dt, n, n, 0, rp.ctypes.data_as(C.c_void_p), ci.ctypes.data_as(C.c_void_p), vv.ctypes.data_as(C.c_void_p), C.byref(A)) == 0
    is_pat = lib.hipk_csr_format(A) == 2
    assert is_pat == (case != "random")
    ld = n + 2
    V = rng.standard_normal((k, ld)).astype(npdt); Q = rng.standard_normal((L, ld)).astype(npdt)
    r = rng.standard_normal((1, ld)).astype(npdt)
    v, q, rr = side.arr(V), side.arr(Q), side.arr(r)
    segs = segs_array(side, [(v, 0, ld, k), (q, 0, ld, L)])
    nov = k + L; nfov = 2 * nov + 1; ALPHA = 100
    fov0 = np.zeros(128); fov0[:nov] = rng.standard_normal(nov) * 1e-2; fov0[nov] = 0.4; fov0[nov + 1:nfov] = rng.standard_normal(nov)
    # a Rayleigh-Ritz decomposition for the step that rides on the last launch
    Hk = rng.standard_normal((k, k)); Hk = (Hk + Hk.T) / 2 + np.diag(np.linspace(-2.0, 3.0, k))
    th, Y = np.linalg.eigh(Hk)
    inp = F.HipkRrIn()
    inp.k, inp.L, inp.cand, inp.largest, inp.grow_row = k, L, 0, 0, 1
    for i in range(k):
        inp.theta[i] = th[i]
        for rw in range(k): inp.Y[rw + i * k] = Y[rw, i]
    G = rng.standard_normal((k, L)) * 0.1
    for l in range(L):
        for j in range(k): inp.G[j + l * k] = G[j, l]
    res = {}
    for mode in ("separate", "deferred"):
        fov = side.arr(fov0); t = side.arr(np.zeros((1, ld), npdt)); xo = side.arr(np.full((1, ld), np.nan, npdt))
        y = side.arr(np.full((1, ld), np.nan, npdt)); hn = side.arr(np.zeros(64)); hn2 = side.arr(np.zeros(64))
        if mode == "deferred":
            assert lib.hipk_tail_defer(side.ctx, 3) == 3
        assert lib.hipk_panel_project_to(side.ctx, dt, n, segs, 2, side.ptr(fov), nov, side.ptr(rr), ld, side.ptr(t), ld, 1, side.ptr(fov, nfov)) == 0
        if mode == "deferred": assert lib.hipk_tail_pending(side.ctx) == 1
        assert lib.hipk_csr_matvec_scaled(A, side.ctx, side.ptr(t), side.ptr(fov, nfov), side.ptr(xo), side.ptr(y), side.ptr(fov, ALPHA)) == 0
        if mode == "deferred": assert lib.hipk_tail_pending(side.ctx) == (3 if is_pat else 2)
        assert lib.hipk_tail_finish(side.ctx, C.byref(inp), side.ptr(fov), nfov, side.ptr(fov, ALPHA), side.ptr(hn)) == 0
        assert lib.hipk_tail_pending(side.ctx) == 0
        # the step as a launch of its own on what is in HBM now
        assert lib.hipk_rr_arrow(side.ctx, C.byref(inp), side.ptr(fov), nfov, side.ptr(fov, ALPHA), side.ptr(hn2)) == 0
        f = side.get(fov)
        res[mode] = dict(n2=f[nfov], dot=f[ALPHA], t=side.get(t)[0, :n].astype(np.float64), xo=side.get(xo)[0, :n], y=side.get(y)[0, :n], hn=side.get(hn), hn2=side.get(hn2))
    lib.hipk_csr_destroy(A)
    side.close()
    eps = 2.3e-16 if dt == F.HIPK_F64 else 1.2e-7
    for mode, d in res.items():
        assert np.array_equal(d["hn"][:34], d["hn2"][:34]), mode                     # the step: same bits either way
        assert d["hn"][33] == 0.0
        a = 1.0 / np.sqrt(d["n2"])
        assert np.array_equal(d["xo"], (a * d["t"]).astype(npdt)), mode              # scaled with the PUBLISHED |t|^2
        assert abs(d["n2"] - float(d["t"] @ d["t"])) <= 50 * eps * d["n2"], mode
        assert abs(d["dot"] - float(d["xo"].astype(np.float64) @ d["y"].astype(np.float64))) <= 200 * eps * np.sqrt(n) * max(1.0, abs(d["dot"])), mode
    s_, d_ = res["separate"], res["deferred"]
    assert np.array_equal(s_["t"], d_["t"])
    assert abs(s_["n2"] - d_["n2"]) <= 4 * 2.3e-16 * s_["n2"]
    if not is_pat:
        assert s_["n2"] == d_["n2"] and np.array_equal(s_["y"], d_["y"]) and s_["dot"] == d_["dot"]      # only the launch count differs
    else:
        assert np.max(np.abs(s_["y"].astype(np.float64) - d_["y"].astype(np.float64))) <= 8 * eps * np.abs(s_["y"]).max()
        assert abs(s_["dot"] - d_["dot"]) <= 100 * eps * np.sqrt(n) * max(1.0, abs(s_["dot"]))


def _lattice_csr(n, rng):
    """a 1-D lattice operator with second-neighbour hopping and two site types: 3 x 2 row patterns away from the ends"""
    rows, cols, vals = [], [], []
    for i in range(n):
        for d, v in ((-2, 0.25), (-1, -1.0), (0, 2.0 + 0.5 * (i % 2)), (1, -1.0), (2, 0.25)):
            if 0 <= i + d < n:
                rows.append(i); cols.append(i + d); vals.append(v)
    rp = np.zeros(n + 1, dtype=np.int64); np.add.at(rp, np.array(rows) + 1, 1)
    return np.cumsum(rp).astype(np.int32), np.array(cols, dtype=np.int32), np.array(vals)


def _lattice8_csr(n):
    """a non-symmetric 1-D lattice operator with the neighbours -4 .. 3, eight different values in a row (all exact in float) and
    two alternating site types: the widest row-pattern table (8 entries), 2 patterns away from the ends"""
    i = np.arange(n)[:, None]
    d = np.arange(-4, 4)[None, :]
    vals = np.array([0.25, -0.5, 0.75, -1.0, 2.0, -1.25, 0.375, -0.625]) + 0 * i
    vals[:, 4] += 0.5 * (i[:, 0] % 2)
    vals[:, 7] -= 0.25 * (i[:, 0] % 2)
    keep = (i + d >= 0) & (i + d < n)
    rp = np.zeros(n + 1, dtype=np.int64); np.cumsum(keep.sum(axis=1), out=rp[1:])
    return rp.astype(np.int32), (i + d)[keep].astype(np.int32), vals[keep]


@pytest.mark.parametrize("dt", [F.HIPK_F64, F.HIPK_F32])
@pytest.mark.parametrize("case", ["lap1d", "lap1d_full_chunks", "lap2d", "lap2d_full_chunks", "lap2d_big", "lap3d", "lattice", "lattice8", "lap3d_slab", "random"])
def test_csr_row_pattern_form(built, dt, case):
    """Matrices whose rows repeat are served by the row-pattern form (csrc/hipk_sparse_pat.hip: one byte per row + a pattern
    table, one lane per row) for one-column products.  Checked: hipk_csr_create picks it for stencils / lattice operators
    and not for a random matrix; y is BIT-IDENTICAL to the CSR tile kernel's (same products, same order, no contraction),
    plain and fused, with and without halo rows; the fused form's normalised vector is bit-identical and its inner product
    agrees to rounding; both agree with numpy."""
    npdt = NPDT[dt]
    rng = np.random.default_rng(11)
    row0, lo_hi = 0, None
    if case == "lap1d": rp, ci, va, n = problems.laplacian_csr((70001,))
    elif case == "lap1d_full_chunks": rp, ci, va, n = problems.laplacian_csr((8192,))   # no ragged chunk: the last pair (interior row, last row) is in the fast form and its first row references the LAST column
    elif case == "lap2d": rp, ci, va, n = problems.laplacian_csr((37, 41))
    elif case == "lap2d_full_chunks": rp, ci, va, n = problems.laplacian_csr((33, 512))   # n = 33 * 512: full chunks only; row n - 1 - 33 is even and its +33 entry is the last column
    elif case == "lap2d_big": rp, ci, va, n = problems.laplacian_csr((1234, 1111))     # > 2 chunks per workgroup of every XCD
    elif case == "lap3d": rp, ci, va, n = problems.laplacian_csr((64, 65, 66))
    elif case == "lattice": n = 40003; rp, ci, va = _lattice_csr(n, rng)
    elif case == "lattice8": n = 6001; rp, ci, va = _lattice8_csr(n)      # table width 8; 12 chunks on a grid of 8: two trips per workgroup
    elif case == "lap3d_slab":
        dims = (23, 19, 17); n = int(np.prod(dims)); row0 = 2000
        rp, ci, va, _ = problems.laplacian_csr(dims, row0=row0, nrows=3003)
    else:
        n = 5000
        counts = rng.integers(1, 7, size=n)
        rp = np.zeros(n + 1, dtype=np.int64); np.cumsum(counts, out=rp[1:]); rp = rp.astype(np.int32)
        ci = np.concatenate([np.sort(rng.choice(n, size=c, replace=False)) for c in counts]).astype(np.int32)
        va = rng.standard_normal(len(ci))
    nloc = len(rp) - 1
    side = Dev()
    lib = side.lib
    lib.hipk_set_spmv_format.argtypes = [C.c_int]
    lib.hipk_csr_format.argtypes = [C.c_void_p]; lib.hipk_csr_npatterns.argtypes = [C.c_void_p]
    lib.hipk_csr_product_bytes.argtypes = [C.c_void_p, C.c_int]; lib.hipk_csr_product_bytes.restype = C.c_double
    old = lib.hipk_set_spmv_format(1)
    try:
        A = C.c_void_p()
        vv = np.ascontiguousarray(va, dtype=npdt)
        assert lib.hipk_csr_create(side.ctx, dt, nloc, n, row0, rp.ctypes.data_as(C.c_void_p), ci.ctypes.data_as(C.c_void_p),
                                   vv.ctypes.data_as(C.c_void_p), C.byref(A)) == 0
        if case == "random":
            assert lib.hipk_csr_format(A) == 0 and lib.hipk_csr_npatterns(A) == 0
            lib.hipk_csr_destroy(A)
            return
        assert lib.hipk_csr_format(A) == 2
        want_pat = {"lap1d": 3, "lap1d_full_chunks": 3, "lap2d": 9, "lap2d_full_chunks": 9, "lap2d_big": 9, "lap3d": 27, "lattice": 6}.get(case)
        if want_pat: assert lib.hipk_csr_npatterns(A) == want_pat
        es = np.dtype(npdt).itemsize
        assert lib.hipk_csr_product_bytes(A, 1) == nloc * (1 + 3 * es)
        Xg = rng.standard_normal(n) * 2.0                                  # the whole vector; this slab owns [row0, row0 + nloc)
        lo, hi = int(lib.hipk_csr_halo_lo(A)), int(lib.hipk_csr_halo_hi(A))
        x = side.arr(Xg[row0:row0 + nloc].astype(npdt))
        xlo = side.arr(Xg[row0 - lo:row0].astype(npdt) if lo else np.zeros(1, npdt))
        xhi = side.arr(Xg[row0 + nloc:row0 + nloc + hi].astype(npdt) if hi else np.zeros(1, npdt))
        assert lib.hipk_csr_set_halo_ld(A, side.ptr(xlo), max(lo, 1), side.ptr(xhi), max(hi, 1)) == 0
        nn = side.arr(np.array([float(np.sum(Xg ** 2))]))
        got = {}
        for fmt in (1, 0):
            lib.hipk_set_spmv_format(fmt)
            assert lib.hipk_csr_format(A) == (2 if fmt else 0)
            y = side.arr(np.full(nloc, np.nan, npdt)); yf = side.arr(np.full(nloc, np.nan, npdt)); xo = side.arr(np.full(nloc, np.nan, npdt))
            dot = side.arr(np.zeros(1))
            assert lib.hipk_csr_matvec(A, None, side.ptr(x), nloc, side.ptr(y), nloc, 1) == 0
            assert lib.hipk_csr_matvec_scaled(A, side.ctx, side.ptr(x), side.ptr(nn), side.ptr(xo), side.ptr(yf), side.ptr(dot)) == 0
            got[fmt] = [side.get(t) for t in (y, yf, xo, dot)]
        assert lib.hipk_csr_product_bytes(A, 0) > nloc * (1 + 2 * es)      # the tile form streams the nonzeros
        lib.hipk_csr_destroy(A)
    finally:
        lib.hipk_set_spmv_format(old)
        side.close()
    for t in range(3):
        assert not np.any(np.isnan(got[1][t])) and np.array_equal(got[1][t], got[0][t]), (case, t)     # bit for bit
    tol = 1e-12 if dt == F.HIPK_F64 else 2e-4
    assert abs(got[1][3][0] - got[0][3][0]) <= tol * np.sqrt(nloc) * (1 + abs(got[0][3][0]))
    # against numpy on the global matrix rows of this slab
    xin = Xg.astype(npdt).astype(np.float64)
    ref = np.zeros(nloc)
    np.add.at(ref, np.repeat(np.arange(nloc), np.diff(rp)), va.astype(npdt).astype(np.float64) * xin[ci])
    assert np.max(np.abs(got[1][0] - ref)) <= tol * 10 * (1 + np.abs(ref).max())
    a = 1.0 / np.sqrt(float(np.sum(Xg ** 2)))
    assert np.max(np.abs(got[1][1] - a * ref)) <= tol * 10 * (1 + np.abs(a * ref).max())
    assert abs(got[1][3][0] - a * a * float(xin[row0:row0 + nloc] @ ref)) <= tol * 50 * np.sqrt(nloc) * (1 + abs(got[1][3][0]))


def _rect_structured_csr(kind, m):
    """rectangular operators whose rows REPEAT (so the pattern scan would accept them): wide [D D] (m x 2m), m x (m+1)
    bidiagonal, tall [D; D] (2m x m) and a tall bidiagonal (m+1) x m — every row of the wide ones references a column
    >= nrows, the tall ones have fewer columns than rows"""
    rows, cols, vals = [], [], []
    if kind == "wide_DD":
        nr, nc = m, 2 * m
        for i in range(m): rows += [i, i]; cols += [i, i + m]; vals += [2.0, -0.5]
    elif kind == "wide_bidiag":
        nr, nc = m, m + 1
        for i in range(m): rows += [i, i]; cols += [i, i + 1]; vals += [1.0, -1.0]
    elif kind == "tall_DD":
        nr, nc = 2 * m, m
        for i in range(2 * m): rows.append(i); cols.append(i % m); vals.append(1.5 if i < m else -0.25)
    else:
        nr, nc = m + 1, m
        for i in range(m + 1):
            if i < m: rows.append(i); cols.append(i); vals.append(1.0)
            if i > 0: rows.append(i); cols.append(i - 1); vals.append(-1.0)
    order = np.lexsort((cols, rows))
    rows, cols, vals = np.array(rows)[order], np.array(cols)[order], np.array(vals)[order]
    rp = np.zeros(nr + 1, dtype=np.int64); np.add.at(rp, rows + 1, 1)
    return np.cumsum(rp).astype(np.int32), cols.astype(np.int32), vals, nr, nc


@pytest.mark.parametrize("dt", [F.HIPK_F64, F.HIPK_F32])
@pytest.mark.parametrize("kind", ["wide_DD", "wide_bidiag", "tall_DD", "tall_bidiag"])
def test_csr_rect_structured_operator(built, dt, kind):
    """Advisor finding of round 5: hipk_csr_create_rect hands the pattern builder x0 == row0 == 0, and pat_kernel sizes its x
    descriptor from nrows — a wide structured operator (A' of a tall structured matrix in the singular value problem) read
    zeros for every column >= nrows in full chunks, a tall one could read past the end of x.  The pattern form is now built
    for square operators / row slabs only; rectangular structured operators with >= 1024 rows (full 512-row chunks) must give
    the numpy product, one column and a block."""
    npdt = NPDT[dt]
    for m in (1024, 4096 + 512, 20000):
        rp, ci, va, nr, nc = _rect_structured_csr(kind, m)
        rng = np.random.default_rng(m)
        for ncols in (1, 3):
            X = (rng.standard_normal((ncols, nc)) + 3.0).astype(npdt)          # no zeros: a read of 0 cannot pass
            res = []
            for side in (Dev(), Host()):
                A = C.c_void_p()
                vv = np.ascontiguousarray(va, dtype=npdt)
                assert side.lib.hipk_csr_create_rect(side.ctx, dt, nr, nc, rp.ctypes.data_as(C.c_void_p), ci.ctypes.data_as(C.c_void_p),
                                                     vv.ctypes.data_as(C.c_void_p), C.byref(A)) == 0
                if side.name == "hip":
                    side.lib.hipk_csr_format.argtypes = [C.c_void_p]
                    assert side.lib.hipk_csr_format(A) != 2, (kind, m)        # never the row-pattern form
                x = side.arr(X); y = side.arr(np.full((ncols, nr), np.nan, dtype=npdt))
                assert side.lib.hipk_csr_matvec(A, None, side.ptr(x), nc, side.ptr(y), nr, ncols) == 0
                res.append(side.get(y).copy())
                side.lib.hipk_csr_destroy(A)
                side.close()
            ref = problems.csr_matvec_numpy(rp, ci, np.asarray(va).astype(npdt).astype(np.float64), X.T.astype(np.float64)).T
            tol = 1e-13 if dt == F.HIPK_F64 else 1e-5
            assert np.max(np.abs(res[0] - ref)) <= tol * (1 + np.abs(ref).max()), (kind, m, ncols)
            assert np.max(np.abs(res[1] - ref)) <= tol * (1 + np.abs(ref).max()), (kind, m, ncols)


@pytest.mark.parametrize("dt", [F.HIPK_F64, F.HIPK_F32])
def test_panel_project_out_of_place(built, dt):
    """Xout = X - [segs] coef with X untouched (the form that leaves the projected vector in a scratch column)"""
    rng = np.random.default_rng(3)
    npdt = NPDT[dt]
    m, ld, k, L = 70003, 70004, 9, 4
    V = rng.standard_normal((k, ld)).astype(npdt); Q = rng.standard_normal((L, ld)).astype(npdt)
    X = rng.standard_normal((1, ld)).astype(npdt); coef = rng.standard_normal(k + L)
    res = []
    for side in (Dev(), Host()):
        v, q, x, o = side.arr(V), side.arr(Q), side.arr(X), side.arr(np.zeros_like(X))
        cf = side.arr(coef); n2 = side.arr(np.zeros(1))
        segs = segs_array(side, [(v, 0, ld, k), (q, 0, ld, L)])
        assert side.lib.hipk_panel_project_to(side.ctx, dt, m, segs, 2, side.ptr(cf), k + L, side.ptr(x), ld, side.ptr(o), ld, 1, side.ptr(n2)) == 0
        res.append((side.get(x), side.get(o), side.get(n2)))
        side.close()
    tol = 1e-12 if dt == F.HIPK_F64 else 1e-4
    ref = X[0, :m].astype(np.float64) - coef[:k] @ V[:, :m].astype(np.float64) - coef[k:] @ Q[:, :m].astype(np.float64)
    for r in res:
        assert np.array_equal(r[0], X)
        assert np.max(np.abs(r[1][0, :m] - ref)) <= tol * 10 * (1 + np.abs(ref).max())
        assert abs(r[2][0] - np.sum(ref ** 2)) <= tol * 10 * np.sum(ref ** 2)


@pytest.mark.parametrize("dt", [F.HIPK_F64, F.HIPK_F32])
@pytest.mark.parametrize("m,k,L,nx,pad", [(70003, 9, 4, 8, 1), (70002, 24, 0, 4, 2), (1000, 3, 2, 2, 0), (50001, 40, 20, 5, 3), (129, 0, 0, 3, 1)])
def test_panel_project_mul_cholqr_sweep(built, dt, m, k, L, nx, pad):
    """X <- (X - [Q V] coef) M in one pass (the device step of a CholQR / SVQB sweep)"""
    rng = np.random.default_rng(m + nx)
    npdt = NPDT[dt]
    ld = m + pad
    V = rng.standard_normal((max(k, 1), ld)).astype(npdt); Q = rng.standard_normal((max(L, 1), ld)).astype(npdt)
    X = rng.standard_normal((nx, ld)).astype(npdt)
    coef = rng.standard_normal((nx, k + L + 1)) / np.sqrt(k + L + 1); Mr = rng.standard_normal((nx, nx))
    res = []
    for side in (Dev(), Host()):
        v, q, x = side.arr(V), side.arr(Q), side.arr(X)
        cf, mm = side.arr(coef), side.arr(Mr)
        segs = segs_array(side, [(q, 0, ld, L), (v, 0, ld, k)])
        assert side.lib.hipk_panel_project_mul(side.ctx, dt, m, segs, 2, side.ptr(cf), k + L + 1, side.ptr(mm), side.ptr(x), ld, nx) == 0
        res.append(side.get(x)[:, :m])
        side.close()
    B = np.concatenate([Q[:L, :m], V[:k, :m]]).astype(np.float64)
    P = X[:, :m].astype(np.float64) - coef[:, :k + L] @ B                    # rows = columns of the panel
    ref = Mr @ P                                                              # out col c = sum_q P(:,q) M(q,c); Mr[c, q] = M(q, c)
    tol = 1e-12 if dt == F.HIPK_F64 else 2e-4
    assert np.max(np.abs(res[0] - res[1])) <= tol * 10 * (1 + np.abs(ref).max())
    assert np.max(np.abs(res[1] - ref)) <= tol * 10 * (1 + np.abs(ref).max())
    # shapes the single-pass form does not cover are reported, not guessed
    side = Dev()
    x = side.arr(np.zeros((9, 16)))
    segs = segs_array(side, [(x, 0, 16, 0), (x, 0, 16, 0)])
    assert side.lib.hipk_panel_project_mul(side.ctx, dt, 8, segs, 2, side.ptr(x), 1, side.ptr(x), side.ptr(x), 16, 9) == 1
    side.close()


@pytest.mark.parametrize("dims", [(1000,), (123, 77), (31, 29, 37)])
def test_stencil_matches_csr(built, dims):
    dt = F.HIPK_F64
    rp, ci, va, n = problems.laplacian_csr(dims)
    rng = np.random.default_rng(n)
    X = rng.standard_normal((2, n))
    side = Dev()
    A = C.c_void_p(); S = C.c_void_p()
    assert side.lib.hipk_csr_create(side.ctx, dt, n, n, 0, rp.ctypes.data_as(C.c_void_p), ci.ctypes.data_as(C.c_void_p),
                                    va.ctypes.data_as(C.c_void_p), C.byref(A)) == 0
    d = list(dims) + [1, 1]
    assert side.lib.hipk_stencil_create(side.ctx, dt, d[0], d[1], d[2], 0, n, C.byref(S)) == 0
    x = side.arr(X); y1 = side.arr(np.zeros_like(X)); y2 = side.arr(np.zeros_like(X))
    assert side.lib.hipk_csr_matvec(A, None, side.ptr(x), n, side.ptr(y1), n, 2) == 0
    assert side.lib.hipk_csr_matvec(S, None, side.ptr(x), n, side.ptr(y2), n, 2) == 0
    a, b = side.get(y1), side.get(y2)
    assert np.max(np.abs(a - b)) <= 1e-13 * 12
    side.lib.hipk_csr_destroy(A); side.lib.hipk_csr_destroy(S); side.close()


@pytest.mark.parametrize("n", [1, 2, 7, 15, 16, 41, 64])
def test_device_rayleigh_ritz_kernel(built, n):
    """hipk_sym_eig (one-workgroup parallel Jacobi): eigenvalues and vectors of the projected matrix
    against numpy and against the plain-C restatement."""
    rng = np.random.default_rng(n)
    B = rng.standard_normal((n, n))
    A = B + B.T + np.diag(np.arange(n) * 3.0)
    w = np.linalg.eigvalsh(A)
    for side in (Dev(), Host()):
        Af = np.asfortranarray(np.triu(A))            # upper triangle only is referenced
        ev = np.zeros(n); Z = np.zeros((n, n), order="F")
        rc = side.lib.hipk_sym_eig(side.ctx, n, Af.ctypes.data_as(C.c_void_p), n, ev.ctypes.data_as(C.c_void_p),
                                   Z.ctypes.data_as(C.c_void_p), n)
        assert rc == 0
        scale = max(1.0, np.abs(w).max())
        assert np.max(np.abs(ev - w)) <= 1e-13 * scale * n
        assert np.linalg.norm(Z.T @ Z - np.eye(n)) <= 1e-13 * n
        assert np.linalg.norm(A @ Z - Z * ev) <= 1e-12 * scale * n
        side.close()


@pytest.mark.parametrize("dt", [F.HIPK_F64, F.HIPK_F32])
@pytest.mark.parametrize("dims,nslabs", [((60, 70), 2), ((23, 19, 17), 3), ((5000,), 4)])
def test_csr_row_slabs_with_halo(built, dt, dims, nslabs):
    """What a row-partitioned run asks of the SpMV kernels, on ONE device: every slab of rows is its own hipk_csr with
    GLOBAL column numbers, its input vector is the local slab plus the two halo buffers the neighbours would send
    (filled by hand here), in the plain form (1 and 3 columns) and in the fused form (scale + A t + t'At) of the
    iteration tail; against the whole-matrix product in numpy and against the oracle's slabs."""
    rng = np.random.default_rng(sum(dims) + nslabs)
    npdt = NPDT[dt]
    n = int(np.prod(dims))
    rp0, ci0, va0, _ = problems.laplacian_csr(dims)
    X = rng.standard_normal((3, n))
    Yref = problems.csr_matvec_numpy(rp0, ci0, va0, X.T).T                     # (3, n)
    tol = 1e-12 if dt == F.HIPK_F64 else 2e-5
    base, rem = divmod(n, nslabs)
    for sidx in range(nslabs):
        nloc = base + (1 if sidx < rem else 0)
        row0 = sidx * base + min(sidx, rem)
        rp, ci, va, _ = problems.laplacian_csr(dims, row0=row0, nrows=nloc)
        outs = []
        for side in (Dev(), Host()):
            A = C.c_void_p()
            assert side.lib.hipk_csr_create(side.ctx, dt, nloc, n, row0, rp.ctypes.data_as(C.c_void_p), ci.ctypes.data_as(C.c_void_p),
                                            np.ascontiguousarray(va, dtype=npdt).ctypes.data_as(C.c_void_p), C.byref(A)) == 0
            lo, hi = int(side.lib.hipk_csr_halo_lo(A)), int(side.lib.hipk_csr_halo_hi(A))
            assert lo == (row0 - int(ci.min()) if row0 > 0 else 0) and hi == max(0, int(ci.max()) - (row0 + nloc) + 1)
            xl = side.arr(X[:, row0:row0 + nloc].astype(npdt))                    # 3 local columns, ld = nloc
            xlo = side.arr(np.ascontiguousarray(X[:, row0 - lo:row0]).astype(npdt) if lo else np.zeros((3, 1), npdt))
            xhi = side.arr(np.ascontiguousarray(X[:, row0 + nloc:row0 + nloc + hi]).astype(npdt) if hi else np.zeros((3, 1), npdt))
            # outputs start as NaN on the device: a row no workgroup wrote shows up as NaN, not as a plausible number
            y = side.arr(np.full((3, nloc), np.nan, npdt))
            assert side.lib.hipk_csr_set_halo_ld(A, side.ptr(xlo), max(lo, 1), side.ptr(xhi), max(hi, 1)) == 0
            assert side.lib.hipk_csr_matvec(A, None, side.ptr(xl), nloc, side.ptr(y), nloc, 3) == 0
            y3 = side.get(y).astype(np.float64)
            y1 = side.arr(np.full((1, nloc), np.nan, npdt))
            assert side.lib.hipk_csr_matvec(A, None, side.ptr(xl), nloc, side.ptr(y1), nloc, 1) == 0
            y1v = side.get(y1).astype(np.float64)
            want1 = Yref[:1, row0:row0 + nloc]
            if not np.max(np.abs(y1v - want1)) <= 50 * tol * max(1.0, np.abs(Yref).max()):
                # the round-2 driver run failed exactly here, once, on bytes that passed on another lease: say what it was
                bad = ~(np.abs(y1v - want1) <= 50 * tol * max(1.0, np.abs(Yref).max()))
                again = side.get(y1).astype(np.float64)
                y1b = side.arr(np.full((1, nloc), np.nan, npdt))
                side.lib.hipk_csr_matvec(A, None, side.ptr(xl), nloc, side.ptr(y1b), nloc, 1)
                rerun = side.get(y1b).astype(np.float64)
                rows = np.nonzero(bad[0])[0]
                pytest.fail(f"{side.name}: one-column halo product wrong in {rows.size} rows [{rows[0]}..{rows[-1]}] of slab {sidx}: "
                            f"got {y1v[0][rows[:4]]}, want {want1[0][rows[:4]]}, NaN (unwritten) {int(np.isnan(y1v[bad]).sum())}; "
                            f"second read-back identical: {np.array_equal(again, y1v, equal_nan=True)}; "
                            f"same launch again correct: {bool(np.max(np.abs(rerun - want1)) <= 50 * tol * max(1.0, np.abs(Yref).max()))}")
            # fused tail on column 0: a = 1/sqrt(norm2), xout = a x, y = A(a x) with the halo entries scaled inside
            red = side.arr(np.array([7.5, 0.0, 0.0]))
            xout = side.arr(np.full((1, nloc), np.nan, npdt)); yf = side.arr(np.full((1, nloc), np.nan, npdt))
            rcf = side.lib.hipk_csr_matvec_scaled(A, side.ctx, side.ptr(xl), side.ptr(red), side.ptr(xout), side.ptr(yf), side.ptr(red, 1))
            assert rcf == 0
            outs.append((y3, y1v, side.get(xout).astype(np.float64), side.get(yf).astype(np.float64), float(side.get(red)[1])))
            side.lib.hipk_csr_destroy(A)
            side.close()
        scale = max(1.0, np.abs(Yref).max())
        a = 1.0 / np.sqrt(7.5)
        for (y3, y1v, xo, yf, dot) in outs:
            assert np.max(np.abs(y3 - Yref[:, row0:row0 + nloc])) <= 50 * tol * scale
            assert np.max(np.abs(y1v[0] - Yref[0, row0:row0 + nloc])) <= 50 * tol * scale
            assert np.max(np.abs(xo[0] - a * X[0, row0:row0 + nloc])) <= 10 * tol * scale
            assert np.max(np.abs(yf[0] - a * Yref[0, row0:row0 + nloc])) <= 50 * tol * scale
            assert abs(dot - a * a * float(X[0, row0:row0 + nloc] @ Yref[0, row0:row0 + nloc])) <= 500 * tol * scale * np.sqrt(nloc)
        assert np.max(np.abs(outs[0][0] - outs[1][0])) <= 50 * tol * scale


@pytest.mark.parametrize("dt", [F.HIPK_F64, F.HIPK_F32])
def test_larnv_stream_on_the_device(built, dt):
    """hipk_larnv_uniform11: the xLARNV(2) stream generated on the device by jumping ahead in the 48-bit congruential
    sequence — bit for bit the numbers of the host routine (itself checked against LAPACK in tests/test_dense_host.py),
    the same seed afterwards, consecutive calls continue the stream."""
    npdt = NPDT[dt]
    for n in (1, 63, 4097, 300001):
        outs = []
        for side in (Dev(), Host()):
            seed = (C.c_int64 * 4)(1, 2, 3, 5)
            x = side.arr(np.zeros(n + 7, npdt))
            assert side.lib.hipk_larnv_uniform11(side.ctx, dt, seed, n, side.ptr(x)) == 0
            assert side.lib.hipk_larnv_uniform11(side.ctx, dt, seed, 7, side.ptr(x, n)) == 0
            outs.append((side.get(x), list(seed)))
            side.close()
        assert np.array_equal(outs[0][0], outs[1][0]) and outs[0][1] == outs[1][1]
        assert np.all(np.abs(outs[0][0]) < 1.0) and outs[0][1] != [1, 2, 3, 5]


@pytest.mark.parametrize("dt", [F.HIPK_F64, F.HIPK_F32])
@pytest.mark.parametrize("nx", [1, 5, 8])
def test_qmr_step_scalars_on_the_device(built, dt, nx):
    """Round 5: the block QMR step with one host synchronisation.  hipk_axpy_proj_dot_jacobi_dev / hipk_qmr_update_dir_dev evaluate
    alpha = rho_prev / (v'w - (x'w)(v'x)), Theta, c, gamma, eta, beta in the launch, from reductions that are in device memory;
    the host solver evaluates the same expressions on the mirrored values.  Checked: the panels they leave are EXACTLY the ones the
    host-coefficient launches leave when the coefficients are computed here in numpy with every operation rounded on its own
    (device == host arithmetic for the scalars), a column with an unusable alpha is left alone, device == oracle."""
    rng = np.random.default_rng(177 + nx)
    npdt = NPDT[dt]
    m, ld = 50021, 50024
    X, W, G, D, De, So = (rng.standard_normal((nx, ld)).astype(npdt) for _ in range(6))
    diag = (2.0 + rng.random(m)).astype(npdt)
    sh = np.resize(np.array([1.0, 0.3, -2.0, 0.0, 1.5]), nx)
    tri = rng.standard_normal(3 * nx) * 3.0
    if nx >= 5:
        tri[nx + 2] = tri[2] * tri[2 * nx + 2]              # sigma == 0 exactly: column 2 leaves the block
    rho_prev, tau_prev, th_prev = np.abs(rng.standard_normal(nx)) + 0.1, np.abs(rng.standard_normal(nx)) + 0.1, np.abs(rng.standard_normal(nx))
    eps = 2.220446049250313e-16
    a = lambda v: (C.c_double * nx)(*v)
    out = []
    for side in (Dev(), Host()):
        x, w, g, d, de, so, dg = (side.arr(t) for t in (X, W, G, D, De, So, diag))
        t3, o2, o1 = side.arr(tri), side.arr(np.zeros(2 * nx)), side.arr(np.zeros(nx))
        assert side.lib.hipk_axpy_proj_dot_jacobi_dev(side.ctx, dt, m, nx, side.ptr(t3), a(rho_prev), C.c_double(eps), side.ptr(w), ld, side.ptr(x), ld,
                                                      side.ptr(g), ld, side.ptr(dg), a(sh), C.c_double(1e-10), side.ptr(o2)) == 0
        assert side.lib.hipk_qmr_update_dir_dev(side.ctx, dt, m, nx, side.ptr(t3), side.ptr(o2), a(rho_prev), a(tau_prev), a(th_prev), C.c_double(eps),
                                                side.ptr(d), ld, side.ptr(de), ld, side.ptr(so), ld, side.ptr(g), ld, side.ptr(dg), a(sh),
                                                C.c_double(1e-10), side.ptr(o1)) == 0
        dev = [side.get(t).copy() for t in (g, d, de, so, o2, o1)]
        # the same step with the coefficients formed on the host (numpy float64: one rounding per operation), from the reductions
        # the first launch left
        ggr = dev[4]
        sigma = tri[nx:2 * nx] - tri[:nx] * tri[2 * nx:]
        with np.errstate(divide="ignore", invalid="ignore"):
            alpha = rho_prev / sigma
        bad = ~np.isfinite(sigma) | (sigma == 0.0) | ~np.isfinite(alpha) | (np.abs(alpha) < eps) | (np.abs(alpha) > 1.0 / eps)
        alpha = np.where(bad, 0.0, alpha)
        g2, d2, de2, so2 = (side.arr(t) for t in (G, D, De, So))
        p2, p1 = side.arr(np.zeros(2 * nx)), side.arr(np.zeros(nx))
        assert side.lib.hipk_axpy_proj_dot_jacobi(side.ctx, dt, m, nx, a(alpha), a(tri[:nx]), side.ptr(w), ld, side.ptr(x), ld, side.ptr(g2), ld,
                                                  side.ptr(dg), a(sh), C.c_double(1e-10), side.ptr(p2)) == 0
        assert np.array_equal(side.get(p2), ggr) and np.array_equal(side.get(g2), dev[0])
        theta = np.sqrt(ggr[:nx]) / tau_prev
        c = 1.0 / np.sqrt(1 + theta * theta)
        gam, eta, beta = ((c * c) * th_prev) * th_prev, (alpha * c) * c, ggr[nx:] / rho_prev
        live = np.nonzero(~bad)[0]
        for col in live:                                    # column by column: the dropped ones are not touched
            one = lambda v: (C.c_double * 1)(v[col])
            off = lambda t: side.ptr(t, int(col) * ld)
            q1 = side.arr(np.zeros(1))
            assert side.lib.hipk_qmr_update_dir(side.ctx, dt, m, 1, one(gam), one(eta), one(beta), off(d2), ld, off(de2), ld, off(so2), ld, off(g2), ld,
                                                side.ptr(dg), one(sh), C.c_double(1e-10), side.ptr(q1)) == 0
        host = [side.get(t).copy() for t in (g2, d2, de2, so2)]
        for t in range(4):
            assert np.array_equal(dev[t], host[t]), t
        if nx >= 5:
            assert bad[2] and np.array_equal(dev[1][2], D[2]) and np.array_equal(dev[3][2], So[2]) and dev[5][2] == 0.0
        out.append(dev)
        side.close()
    tol = 1e-12 if dt == F.HIPK_F64 else 2e-4
    for t in range(4):                                      # device == oracle
        assert np.max(np.abs(out[0][t][:, :m] - out[1][t][:, :m]) / (1 + np.abs(out[1][t][:, :m]))) <= tol * 10
    for t in (4, 5):
        assert np.max(np.abs(out[0][t] - out[1][t]) / (1 + np.abs(out[1][t]))) <= tol * np.sqrt(m)
