"""The device pieces of the geometric multigrid preconditioner (csrc/hipk_mg.hip, primme_amd_multigrid_precond in
csrc/amd_operator.hip) against the numpy restatement of tests/mg_cases.py, at the smallest shapes that can go wrong.

hipk_mg_stencil_step, hipk_mg_restrict, hipk_mg_prolong_add: x-lengths 1, 2, 3, 63, 64, 65, 129 (below, at and above a wave,
across a workgroup's first trip), odd and even lengths in every coarsened dimension, a dimension of 2 that is kept, 2-D and 3-D,
1, 3 and 8 columns, leading dimension m (16-byte accesses when m allows), m + 1 (odd: the element path) and m + 8, Out on Yprev,
Yk = NULL, Yprev = NULL, double and float.  Panels are NaN outside the block (padding rows, the column behind it), so an access
outside shows.  Every output is a sum of at most 27 products that the kernels accumulate in double and round once to the panel
type: per element |out - ref| <= 32 eps sum |terms|, eps of the panel type, ref and the terms in float64 from the inputs as
rounded to the panel type.  The adjoint identity <R f, c> = 2^-dc <f, P c> (dc coarsened dimensions) is checked on the DEVICE's
outputs, to the two bounds added.

The whole application K^-1 x on (6, 7, 1), (33, 35, 1), (9, 8, 7), (65, 3, 2) against the numpy V-cycle: the difference to the
V-cycle in longdouble is at most 64 x what the SAME V-cycle in float64 differs from it (the reference's own rounding level;
floor 1e-13 relative); in float the pair is float64 / float32.  Device symmetry X'(K Y) = (K X)'Y, and the return codes of
primme_amd_operator_set_multigrid, which launch nothing."""
import ctypes as C

import numpy as np
import pytest

import mg_cases as MG
from kernel_harness import Dev, NPDT
from primme_amd import _ffi as F

pytestmark = pytest.mark.gpu
DTYPES = [F.HIPK_F64, F.HIPK_F32]
EPS = {F.HIPK_F64: 2.0 ** -52, F.HIPK_F32: 2.0 ** -23}
STEP_GRIDS = [(1, 1, 1), (2, 1, 1), (3, 4, 1), (63, 5, 1), (64, 3, 2), (65, 2, 3), (129, 7, 1), (129, 3, 5), (1, 9, 4), (2, 2, 2)]
FINE_GRIDS = [(1, 7, 1), (2, 6, 5), (3, 2, 1), (63, 4, 3), (64, 5, 2), (65, 3, 2), (129, 6, 1), (129, 5, 4), (6, 7, 1), (9, 8, 7)]
NCOLS = (1, 3, 8)
LDOFF = (0, 1, 8)
APPLY_GRIDS = [(6, 7, 1), (33, 35, 1), (9, 8, 7), (65, 3, 2)]


@pytest.fixture(scope="module")
def dev(built):
    d = Dev()
    yield d
    d.close()


def _stream(dev):
    return C.c_void_p(dev.lib.hipk_ctx_stream(dev.ctx))


def _i3(n):
    return (C.c_int * 3)(*n)


def _panel(dev, rng, m, nc, ld, npdt, fill=None):
    """(host values [nc, m] as rounded to the panel type, device panel of nc + 1 columns of ld elements, NaN outside the block)"""
    h = np.full((nc + 1, ld), np.nan, dtype=npdt)
    h[:nc, :m] = rng.standard_normal((nc, m)) if fill is None else fill
    return h[:nc, :m].astype(np.float64), dev.arr(h)


def _block(dev, t, m, nc):
    """the block of a device panel, after checking that nothing outside it was written"""
    h = dev.get(t)
    assert np.all(np.isnan(h[nc:])) and np.all(np.isnan(h[:nc, m:]))
    return h[:nc, :m].astype(np.float64)


def _stencil_terms(n, w, yk):
    """(sum_d w_d L_d yk, sum of the absolute values of its terms) for a block [nc, m]"""
    nc = yk.shape[0]
    g = yk.reshape(nc, n[2], n[1], n[0])
    lap, mag = np.zeros_like(g), np.zeros_like(g)
    for d, ax in ((0, 3), (1, 2), (2, 1)):
        if n[d] == 1:
            continue
        p = np.zeros((nc, n[2] + 2, n[1] + 2, n[0] + 2))
        p[:, 1:-1, 1:-1, 1:-1] = g
        lo = [slice(None), slice(1, -1), slice(1, -1), slice(1, -1)]
        hi = list(lo)
        lo[ax], hi[ax] = slice(0, -2), slice(2, None)
        lap += w[d] * (2 * g - p[tuple(lo)] - p[tuple(hi)])
        mag += abs(w[d]) * (2 * np.abs(g) + np.abs(p[tuple(lo)]) + np.abs(p[tuple(hi)]))
    return lap.reshape(nc, -1), mag.reshape(nc, -1)


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("n", STEP_GRIDS)
def test_stencil_step(dev, n, dt):
    npdt, lib = NPDT[dt], dev.lib
    m = int(np.prod(n))
    rng = np.random.default_rng(m + dt)
    w = (0.7, 1.3, 0.4) if m % 2 else (1.0, 0.25, 0.0625)
    worst = 0.0
    for nc in NCOLS:
        for off in LDOFF:
            lds = [m + off] * 4
            cf = F.HipkChebCoef()
            for c in range(8):
                cf.cy[c], cf.cp[c], cf.cx[c], cf.cw[c] = 1.1 + 0.1 * c, -0.6 - 0.05 * c, 0.8 + 0.03 * c, -0.45 + 0.02 * c
            col = lambda a: np.array(a[:nc])[:, None]
            for variant in ("apart", "out_on_yprev", "no_yk", "no_yprev"):
                x, dx = _panel(dev, rng, m, nc, lds[0], npdt)
                yk, dk = _panel(dev, rng, m, nc, lds[1], npdt)
                yp, dp = _panel(dev, rng, m, nc, lds[2], npdt)
                _, do = _panel(dev, rng, m, nc, lds[3], npdt)
                has_k, has_p = variant != "no_yk", variant != "no_yprev"
                out, ldo = (dp, lds[2]) if variant == "out_on_yprev" else (do, lds[3])
                rc = lib.hipk_mg_stencil_step(_stream(dev), dt, _i3(n), (C.c_double * 3)(*w), nc, C.byref(cf), dev.ptr(dx), lds[0],
                                              dev.ptr(dk) if has_k else None, lds[1], dev.ptr(dp) if has_p else None, lds[2],
                                              dev.ptr(out), ldo)
                assert rc == 0, (variant, nc, off)
                ref, mag = col(cf.cx) * x, np.abs(col(cf.cx) * x)
                if has_k:
                    lap, lmag = _stencil_terms(n, w, yk)
                    ref = ref + col(cf.cy) * yk + col(cf.cw) * lap
                    mag = mag + np.abs(col(cf.cy) * yk) + np.abs(col(cf.cw)) * lmag
                if has_p:
                    ref, mag = ref + col(cf.cp) * yp, mag + np.abs(col(cf.cp) * yp)
                got = _block(dev, out, m, nc)
                ratio = np.abs(got - ref) / (32 * EPS[dt] * mag)
                assert ratio.max() <= 1.0, (variant, nc, off, float(ratio.max()))
                worst = max(worst, float(ratio.max()))
                if variant != "out_on_yprev":
                    assert np.array_equal(_block(dev, dp, m, nc), yp)          # the inputs are left alone
                assert np.array_equal(_block(dev, dk, m, nc), yk)
    print(f"stencil step {n} {npdt.__name__}: largest |out - ref| / (32 eps sum|terms|) = {worst:.3f}")


def _coarse(nf):
    return tuple(d // 2 if d >= 3 else d for d in nf)


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("nf", FINE_GRIDS)
def test_restrict_prolong_and_adjoint(dev, nf, dt):
    npdt, lib = NPDT[dt], dev.lib
    nc3 = _coarse(nf)
    mf, mc = int(np.prod(nf)), int(np.prod(nc3))
    dc = sum(MG.coarsened(nf))
    R, P = MG.restriction(nf), MG.prolongation(nf)
    rng = np.random.default_rng(mf + 7 * dt)
    worst = [0.0, 0.0, 0.0]
    for nc in NCOLS:
        for off in LDOFF:
            ldf, ldc = mf + off, mc + off
            f, df = _panel(dev, rng, mf, nc, ldf, npdt)
            _, dcoarse = _panel(dev, rng, mc, nc, ldc, npdt)
            assert lib.hipk_mg_restrict(_stream(dev), dt, _i3(nf), _i3(nc3), nc, dev.ptr(df), ldf, dev.ptr(dcoarse), ldc) == 0
            rf = _block(dev, dcoarse, mc, nc)
            ratio = np.abs(rf - f @ R.T) / np.maximum(32 * EPS[dt] * (np.abs(f) @ np.abs(R).T), np.finfo(np.float64).tiny)
            assert ratio.max() <= 1.0, ("restrict", nc, off, float(ratio.max()))
            worst[0] = max(worst[0], float(ratio.max()))
            assert np.array_equal(_block(dev, df, mf, nc), f)
            # Y += P C, on a random Y and on zero (the second gives P c itself for the adjoint identity)
            c, dcc = _panel(dev, rng, mc, nc, ldc, npdt)
            y, dy = _panel(dev, rng, mf, nc, ldf, npdt)
            _, dz = _panel(dev, rng, mf, nc, ldf, npdt, fill=0.0)
            assert lib.hipk_mg_prolong_add(_stream(dev), dt, _i3(nf), _i3(nc3), nc, dev.ptr(dcc), ldc, dev.ptr(dy), ldf) == 0
            assert lib.hipk_mg_prolong_add(_stream(dev), dt, _i3(nf), _i3(nc3), nc, dev.ptr(dcc), ldc, dev.ptr(dz), ldf) == 0
            ratio = np.abs(_block(dev, dy, mf, nc) - (y + c @ P.T)) / (32 * EPS[dt] * (np.abs(y) + np.abs(c) @ np.abs(P).T))
            assert ratio.max() <= 1.0, ("prolong", nc, off, float(ratio.max()))
            worst[1] = max(worst[1], float(ratio.max()))
            pc = _block(dev, dz, mf, nc)
            assert np.array_equal(_block(dev, dcc, mc, nc), c)
            # <R f, c> = 2^-dc <f, P c> from the device's R f and P c; the sums in longdouble, so that the two kernels' bounds are
            # all that is allowed: 32 eps (|c|'|R||f| + 2^-dc |f|'|P||c|) = 64 eps |c|'|R||f|
            L = np.longdouble
            lhs = np.sum(rf.astype(L) * c.astype(L), axis=1)
            rhs = np.sum(f.astype(L) * pc.astype(L), axis=1) * L(2.0 ** -dc)
            bound = 64 * EPS[dt] * np.sum((np.abs(f) @ np.abs(R).T) * np.abs(c), axis=1)
            ratio = np.abs(lhs - rhs).astype(np.float64) / bound
            assert ratio.max() <= 1.0, ("adjoint", nc, off, float(ratio.max()))
            worst[2] = max(worst[2], float(ratio.max()))
    print(f"{nf} -> {nc3} {npdt.__name__}: restrict {worst[0]:.3f}, prolong {worst[1]:.3f}, adjoint {worst[2]:.3f} of the bound")


def test_kernel_argument_errors(dev):
    lib, st = dev.lib, _stream(dev)
    rng = np.random.default_rng(1)
    _, a = _panel(dev, rng, 12, 1, 12, np.float64)
    _, b = _panel(dev, rng, 12, 1, 12, np.float64)
    cf = F.HipkChebCoef()
    w = (C.c_double * 3)(1, 1, 1)
    args = (dev.ptr(a), 12, dev.ptr(b), 12, None, 0)
    for cdt in (F.HIPK_C64, F.HIPK_C32):
        assert lib.hipk_mg_stencil_step(st, cdt, _i3((4, 3, 1)), w, 1, C.byref(cf), *args, dev.ptr(a), 12) == -44
        assert lib.hipk_mg_restrict(st, cdt, _i3((4, 3, 1)), _i3((2, 1, 1)), 1, dev.ptr(a), 12, dev.ptr(b), 12) == -44
        assert lib.hipk_mg_prolong_add(st, cdt, _i3((4, 3, 1)), _i3((2, 1, 1)), 1, dev.ptr(b), 12, dev.ptr(a), 12) == -44
    assert lib.hipk_mg_stencil_step(st, F.HIPK_F64, _i3((4, 3, 1)), w, 9, C.byref(cf), *args, dev.ptr(a), 12) == -1     # 9 columns
    assert lib.hipk_mg_stencil_step(st, F.HIPK_F64, _i3((4, 0, 1)), w, 1, C.byref(cf), *args, dev.ptr(a), 12) == -1
    assert lib.hipk_mg_stencil_step(st, F.HIPK_F64, _i3((4, 3, 1)), w, 1, C.byref(cf), *args, dev.ptr(b), 12) == -1     # Out on Yk
    assert lib.hipk_mg_restrict(st, F.HIPK_F64, _i3((4, 3, 1)), _i3((2, 3, 1)), 1, dev.ptr(a), 12, dev.ptr(b), 12) == -1   # 3 -> 1
    assert lib.hipk_mg_prolong_add(st, F.HIPK_F64, _i3((4, 3, 1)), _i3((4, 1, 1)), 1, dev.ptr(b), 12, dev.ptr(a), 12) == -1


# ---- the whole application ------------------------------------------------------------------------------------------
_hier = {}


def _reference(dims, shift, x, types=(np.longdouble, np.float64, np.float32)):
    """the numpy V-cycle of the block x [m, k] in longdouble, float64 and float32; the dense hierarchies are built once"""
    out = []
    for t in types:
        if (dims, shift, t) not in _hier:
            _hier[(dims, shift, t)] = MG.Hierarchy(dims, shift=shift, dt=t)
        out.append(_hier[(dims, shift, t)].vcycle(x.astype(t)))
    return tuple(out)


class _Op:
    """a stencil operator of the grid with the multigrid preconditioner configured, and the callback's parameter block"""

    def __init__(self, dev, dims, dt, shift=0.0, nu=2, ncs=16, scale=1.0):
        self.dev, lib = dev, dev.lib
        m = int(np.prod(dims))
        self.A, self.op = C.c_void_p(), C.c_void_p()
        assert lib.hipk_stencil_create(dev.ctx, dt, dims[0], dims[1], dims[2], 0, m, C.byref(self.A)) == 0
        assert lib.primme_amd_operator_create(C.byref(self.op), self.A, None) == 0
        assert lib.primme_amd_operator_set_multigrid(self.op, dims[0], dims[1], dims[2], nu, ncs, scale, shift) == 0
        self.p = F.PrimmeParams()
        self.p.preconditioner = self.op
        self.m, self.dt = m, dt

    def apply(self, x, ldx, ldy, rng):
        """K^-1 x for a host block x [m, k] -> [m, k]"""
        k = x.shape[1]
        npdt = NPDT[self.dt]
        _, dx = _panel(self.dev, rng, self.m, k, ldx, npdt, fill=x.T)
        _, dy = _panel(self.dev, rng, self.m, k, ldy, npdt)
        lx, ly, bs, ierr = F.PRIMME_INT(ldx), F.PRIMME_INT(ldy), C.c_int(k), C.c_int(-1)
        self.dev.lib.primme_amd_multigrid_precond(self.dev.ptr(dx), C.byref(lx), self.dev.ptr(dy), C.byref(ly), C.byref(bs), C.byref(self.p),
                                                  C.byref(ierr))
        assert ierr.value == 0
        return _block(self.dev, dy, self.m, k).T

    def close(self):
        self.dev.lib.primme_amd_operator_destroy(self.op)
        self.dev.lib.hipk_csr_destroy(self.A)


@pytest.mark.parametrize("shift", [0.0, 0.5])
@pytest.mark.parametrize("dims", APPLY_GRIDS)
def test_application_against_numpy_vcycle(dev, dims, shift):
    m = int(np.prod(dims))
    rng = np.random.default_rng(m)
    x = rng.standard_normal((m, 3)).astype(np.float32).astype(np.float64)       # the same block in every precision
    vl, v64, v32 = _reference(dims, shift, x)
    scale = float(np.abs(vl).max())
    for dt, ref, own in ((F.HIPK_F64, vl, np.abs(v64 - vl).max()), (F.HIPK_F32, v64, np.abs(v32.astype(np.float64) - v64).max())):
        tol = 64 * float(own) if dt == F.HIPK_F32 else max(64 * float(own), 1e-13 * scale)
        op = _Op(dev, dims, dt, shift=shift)
        try:
            dev.lib.primme_amd_multigrid_stats(None, None)
            got = op.apply(x, m + 1, m, rng)
            ap, la = C.c_long(0), C.c_long(0)
            dev.lib.primme_amd_multigrid_stats(C.byref(ap), C.byref(la))
        finally:
            op.close()
        err = float(np.abs(got - ref.astype(np.float64)).max())
        print(f"{dims} shift {shift} {NPDT[dt].__name__}: |device - reference| = {err:.3e}, the reference's own rounding {float(own):.3e} "
              f"(ratio {err / float(own):.2f}), |K^-1 x| = {scale:.3e}; {la.value} launches")
        assert err <= tol
        # V(2, 2) with 16 coarse steps: 6 launches per level but the last, 15 there
        levels = len(MG.plan(dims)[0])
        assert ap.value == 3 and la.value == 6 * (levels - 1) + 15


@pytest.mark.parametrize("dt", DTYPES)
def test_wide_block_is_chunked_and_steps_vary(dev, dt):
    """11 columns (a chunk of 8 and one of 3) with V(3, 3) and 5 coarse steps, and V(1, 1) with 1: the panel bookkeeping for odd
    and single step counts, against the float64 V-cycle to the float32 / float64 tolerance of the test above"""
    dims = (9, 8, 7)
    m = int(np.prod(dims))
    rng = np.random.default_rng(3)
    x = rng.standard_normal((m, 11)).astype(np.float32).astype(np.float64)
    for nu, ncs in ((3, 5), (1, 1), (2, 2)):
        vl = MG.Hierarchy(dims, nu, ncs, 1.5, 0.25, dt=np.longdouble).vcycle(x.astype(np.longdouble))
        lo_t = np.float64 if dt == F.HIPK_F64 else np.float32
        own = np.abs(MG.Hierarchy(dims, nu, ncs, 1.5, 0.25, dt=lo_t).vcycle(x.astype(lo_t)).astype(np.longdouble) - vl).max()
        op = _Op(dev, dims, dt, shift=0.25, nu=nu, ncs=ncs, scale=1.5)
        try:
            got = op.apply(x, m, m + 3, rng)
        finally:
            op.close()
        err = float(np.abs(got - vl.astype(np.float64)).max())
        assert err <= max(64 * float(own), 1e-13 * float(np.abs(vl).max())), (nu, ncs, err, float(own))


@pytest.mark.parametrize("dims", [(33, 35, 1), (9, 8, 7)])
def test_device_symmetry(dev, dims):
    """X'(K Y) = (K X)'Y: each side carries the application's error (at most the tolerance above, per element) against the
    other block"""
    m = int(np.prod(dims))
    rng = np.random.default_rng(m + 1)
    X, Y = rng.standard_normal((m, 3)), rng.standard_normal((m, 3))
    op = _Op(dev, dims, F.HIPK_F64)
    try:
        KX, KY = op.apply(X, m, m, rng), op.apply(Y, m + 1, m + 8, rng)
    finally:
        op.close()
    tol = []
    for B in (X, Y):
        vl, v64 = _reference(dims, 0.0, B, types=(np.longdouble, np.float64))
        tol.append(max(64 * float(np.abs(v64 - vl).max()), 1e-13 * float(np.abs(vl).max())))
    L = np.longdouble
    lhs, rhs = X.astype(L).T @ KY.astype(L), KX.astype(L).T @ Y.astype(L)
    bound = np.abs(X).sum(axis=0)[:, None] * tol[1] + tol[0] * np.abs(Y).sum(axis=0)[None, :]
    assert np.all(np.abs(lhs - rhs).astype(np.float64) <= bound), (np.abs(lhs - rhs).max(), bound.min())


def test_set_multigrid_return_codes(dev):
    lib = dev.lib
    lib.primme_amd_multigrid_stats(None, None)
    A, op = C.c_void_p(), C.c_void_p()
    assert lib.hipk_stencil_create(dev.ctx, F.HIPK_F64, 6, 7, 1, 0, 42, C.byref(A)) == 0
    assert lib.primme_amd_operator_create(C.byref(op), A, None) == 0
    sm = lib.primme_amd_operator_set_multigrid
    assert sm(op, 6, 7, 1, 2, 16, 1.0, 0.0) == 0 and sm(op, 7, 6, 1, 1, 1, 0.5, 2.0) == 0 and sm(op, 42, 1, 1, 2, 16, 1.0, 0.0) == 0
    assert sm(op, 6, 6, 1, 2, 16, 1.0, 0.0) == -1 and sm(op, 6, 7, 0, 2, 16, 1.0, 0.0) == -1 and sm(op, -6, -7, 1, 2, 16, 1.0, 0.0) == -1
    assert sm(op, 6, 7, 1, 0, 16, 1.0, 0.0) == -1 and sm(op, 6, 7, 1, 2, 0, 1.0, 0.0) == -1
    assert sm(op, 6, 7, 1, 2, 16, 0.0, 0.0) == -1 and sm(op, 6, 7, 1, 2, 16, -1.0, 0.0) == -1 and sm(op, 6, 7, 1, 2, 16, float("nan"), 0.0) == -1
    assert sm(op, 6, 7, 1, 2, 16, 1.0, -0.5) == -1 and sm(op, 6, 7, 1, 2, 16, 1.0, float("nan")) == -1
    assert sm(None, 6, 7, 1, 2, 16, 1.0, 0.0) == -1
    # the real-equivalent mode of a Hermitian problem
    assert lib.primme_amd_operator_set_complex(op, 1) == 0 and sm(op, 6, 7, 1, 2, 16, 1.0, 0.0) == -44
    assert lib.primme_amd_operator_set_complex(op, 0) == 0 and sm(op, 6, 7, 1, 2, 16, 1.0, 0.0) == 0
    lib.primme_amd_operator_destroy(op); lib.hipk_csr_destroy(A)
    # one grid point: M = shift
    assert lib.hipk_stencil_create(dev.ctx, F.HIPK_F64, 1, 1, 1, 0, 1, C.byref(A)) == 0
    assert lib.primme_amd_operator_create(C.byref(op), A, None) == 0
    assert sm(op, 1, 1, 1, 2, 16, 1.0, 0.0) == -1 and sm(op, 1, 1, 1, 2, 16, 1.0, 0.5) == 0
    lib.primme_amd_operator_destroy(op); lib.hipk_csr_destroy(A)
    # a complex operator
    rp, ci = np.arange(43, dtype=np.int32), np.arange(42, dtype=np.int32)
    va = np.ones(42, dtype=np.complex128)
    assert lib.hipk_csr_create(dev.ctx, F.HIPK_C64, 42, 42, 0, rp.ctypes.data_as(C.c_void_p), ci.ctypes.data_as(C.c_void_p),
                               va.ctypes.data_as(C.c_void_p), C.byref(A)) == 0
    assert lib.primme_amd_operator_create(C.byref(op), A, None) == 0
    assert sm(op, 6, 7, 1, 2, 16, 1.0, 0.0) == -44
    lib.primme_amd_operator_destroy(op); lib.hipk_csr_destroy(A)
    ap, la = C.c_long(-1), C.c_long(-1)
    lib.primme_amd_multigrid_stats(C.byref(ap), C.byref(la))
    assert (ap.value, la.value) == (0, 0)                    # nothing was launched
