"""hipk_amg_csr_apply (csrc/hipk_amg.hip), the transfer kernel of smoothed aggregation, against numpy, and the whole application
with the smoothed hierarchy against the restatement of tests/amg_smoothed_cases.py.

Out = T In and Out += T In for random CSR matrices T with double values: 1, 63, 64, 65, 64 VW - 1, 64 VW + 1 and 1000 rows
(VW = 2 for double, 4 for float: below, at and above what a wave takes per trip), the columns another number than the rows, the
row lengths drawn from 0, 1, 2, 64, 65 and 200 (at most 64: the lane's own sum, more: the wave's), shuffled so that the rows of a
lane mix both kinds; one matrix of long rows only and one of empty rows only; 1, 3 and 8 columns, both dtypes, the three panel
layouts of test_amg_kernels_gpu.py (16-byte accesses; odd leading dimension and offset base: the element path).  Panels are
NaN outside the block.  Per element |out - ref| <= 32 eps sum |terms|, eps of the panel type, ref and the terms in float64
from the inputs as rounded to the panel type (accumulate: Out's old value is one of the terms).  Two runs give the same bits.

The application K^-1 x on 33 x 35 (shift 0 and 0.5), 9 x 8 x 7 and the four tiles of LUNDA.mtx: the difference to the cycle in
longdouble is at most 64 x what the SAME cycle in float64 differs from it (float: float64 / float32), the margin of
test_amg_kernels_gpu.py::test_application_against_the_restatement.  The ratios measured are in DESIGN.md section 4p."""
import ctypes as C

import numpy as np
import pytest

import amg_cases as AMG
import amg_smoothed_cases as SA
from kernel_harness import Dev, NPDT
from primme_amd import _ffi as F
from primme_amd import problems
from test_amg_kernels_gpu import EPS, LAYOUTS, NCOLS, TINY, _Panel, _ivec, _stream

pytestmark = pytest.mark.gpu
DTYPES = [F.HIPK_F64, F.HIPK_F32]
VW = {F.HIPK_F64: 2, F.HIPK_F32: 4}
LENGTHS = (0, 1, 2, 64, 65, 200)


@pytest.fixture(scope="module")
def dev(built):
    d = Dev()
    yield d
    d.close()


def _random_csr(rng, nrows, ncols, lengths):
    """rows of the given lengths (clipped to ncols), distinct ascending columns in range, normal values"""
    lengths = np.minimum(np.asarray(lengths), ncols)
    rp = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)
    ci = np.concatenate([np.sort(rng.choice(ncols, size=k, replace=False)) for k in lengths] + [np.zeros(0, dtype=np.int64)])
    va = rng.standard_normal(int(rp[-1]))
    assert len(rp) == nrows + 1 and (len(ci) == 0 or (ci.min() >= 0 and ci.max() < ncols))
    return rp, ci.astype(np.int64), va


def _cases(dt):
    vw = VW[dt]
    out = [("mix", m, (m * 3 + 7) // 2 if m != 65 else 300) for m in (1, 63, 64, 65, 64 * vw - 1, 64 * vw + 1, 1000)]
    return out + [("long", 70, 257), ("empty", 130, 5)]


def _run(dev, dt, T, acc, nx, x, y):
    rp, ci, va = T
    return dev.lib.hipk_amg_csr_apply(_stream(dev), dt, y.m, x.m, dev.ptr(rp), dev.ptr(ci), dev.ptr(va), acc, nx, x.ptr, x.ld, y.ptr, y.ld)


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("case", range(9))
def test_csr_apply(dev, case, dt):
    kind, nrows, ncols = _cases(dt)[case]
    npdt = NPDT[dt]
    rng = np.random.default_rng(100 * case + dt)
    if kind == "mix":
        lengths = rng.choice(LENGTHS, size=nrows)
        if nrows >= 63:
            lengths[:6] = LENGTHS                                   # every length is there
            lengths = rng.permutation(lengths)
    else:
        lengths = np.full(nrows, 200 if kind == "long" else 0)
    lengths = np.minimum(lengths, ncols)
    rp, ci, va = _random_csr(rng, nrows, ncols, lengths)
    A = SA.dense_rect(nrows, ncols, rp, ci, va)
    # a NaN behind the arrays: an entry read past the end shows in the sum
    T = (_ivec(dev, rp), _ivec(dev, np.concatenate([ci, [0]])), dev.arr(np.concatenate([va, [np.nan]])))
    worst = 0.0
    for nx in NCOLS:
        for layout in LAYOUTS:
            for acc in (0, 1):
                x = _Panel(dev, rng, ncols, nx, layout, npdt)
                y = _Panel(dev, rng, nrows, nx, layout, npdt)
                assert _run(dev, dt, T, acc, nx, x, y) == 0
                got = y.block()
                ref, mag = x.host @ A.T, np.abs(x.host) @ np.abs(A.T)
                if acc:
                    ref, mag = ref + y.host, mag + np.abs(y.host)
                ratio = np.abs(got - ref) / np.maximum(32 * EPS[dt] * mag, TINY)
                assert ratio.max() <= 1.0, (kind, nrows, nx, layout, acc, float(ratio.max()))
                if not acc:
                    assert np.all(got[:, lengths == 0] == 0.0)      # an empty row stores zero
                worst = max(worst, float(ratio.max()))
                assert np.array_equal(x.block(), x.host)
                # the same again: every sum has one order
                y2 = _Panel(dev, rng, nrows, nx, layout, npdt, fill=y.host)
                assert _run(dev, dt, T, acc, nx, x, y2) == 0
                assert np.array_equal(y2.block().view(np.int64), got.view(np.int64))
    print(f"{kind} {nrows} x {ncols}, {int(rp[-1])} entries, longest row {int(lengths.max())} {npdt.__name__}: "
          f"largest |out - ref| / (32 eps sum|terms|) = {worst:.3f}")


def test_csr_apply_argument_errors(dev):
    lib, st = dev.lib, _stream(dev)
    rng = np.random.default_rng(2)
    rp, ci, va = _random_csr(rng, 12, 7, [2] * 12)
    drp, dci, dva = _ivec(dev, rp), _ivec(dev, ci), dev.arr(va)
    x = _Panel(dev, rng, 7, 9, "aligned", np.float64)
    y = _Panel(dev, rng, 12, 9, "aligned", np.float64)
    P = dev.ptr

    def run(dt=F.HIPK_F64, nrows=12, ncols=7, rp_=P(drp), ci_=P(dci), va_=P(dva), acc=0, nx=1, x_=x.ptr, y_=y.ptr):
        return lib.hipk_amg_csr_apply(st, dt, nrows, ncols, rp_, ci_, va_, acc, nx, x_, x.ld, y_, y.ld)

    for cdt in (F.HIPK_C64, F.HIPK_C32):
        assert run(dt=cdt) == -44
    assert run(nx=0) == 0 and run(nx=-1) == 0                       # nothing to do, as the neighbours answer
    assert run(nx=9) == -1
    assert run(nrows=0) == -1 and run(nrows=-3) == -1 and run(ncols=0) == -1 and run(ncols=-1) == -1
    assert run(nrows=2 ** 31) == -1 and run(ncols=2 ** 31) == -1
    assert run(rp_=None) == -1 and run(ci_=None) == -1 and run(va_=None) == -1 and run(x_=None) == -1 and run(y_=None) == -1
    assert run(y_=x.ptr) == -1 and run(acc=1, y_=x.ptr) == -1
    assert np.array_equal(x.block(), x.host) and np.array_equal(y.block(), y.host)          # nothing was launched
    assert run(nx=8) == 0 and run(acc=1, nx=8) == 0


# ---- the whole application ------------------------------------------------------------------------------------------
def _case(name):
    if name == "lunda_x4":
        rp, ci, va = AMG.lunda_tiled(4)
        return rp, ci, va, 0.0
    dims, shift = {"lap_33x35": ((33, 35), 0.0), "lap_33x35_shift": ((33, 35), 0.5), "lap_9x8x7": ((9, 8, 7), 0.0)}[name]
    rp, ci, va, _ = problems.laplacian_csr(dims)
    return rp, ci, va, shift


class _Op:
    """a CSR operator with the smoothed preconditioner configured, and the callback's parameter block"""

    def __init__(self, dev, rp, ci, va, dt, nu=2, ncs=16, theta=0.08, omega=SA.OMEGA, shift=0.0):
        self.dev, lib = dev, dev.lib
        self.m, self.dt = len(rp) - 1, dt
        rp, ci, va = np.ascontiguousarray(rp, dtype=np.int32), np.ascontiguousarray(ci, dtype=np.int32), np.ascontiguousarray(va, dtype=NPDT[dt])
        self.A, self.op = C.c_void_p(), C.c_void_p()
        self.args = (rp.ctypes.data_as(C.c_void_p), ci.ctypes.data_as(C.c_void_p), va.ctypes.data_as(C.c_void_p))
        self.keep = (rp, ci, va)
        assert lib.hipk_csr_create(dev.ctx, dt, self.m, self.m, 0, *self.args, C.byref(self.A)) == 0
        assert lib.primme_amd_operator_create(C.byref(self.op), self.A, None) == 0
        self.rc = lib.primme_amd_operator_set_amg_smoothed(self.op, *self.args, nu, ncs, theta, omega, shift)
        self.p = F.PrimmeParams()
        self.p.preconditioner = self.op

    def apply(self, x, rng, layouts=("odd_ld", "aligned")):
        k = x.shape[1]
        npdt = NPDT[self.dt]
        dx = _Panel(self.dev, rng, self.m, k, layouts[0], npdt, fill=x.T)
        dy = _Panel(self.dev, rng, self.m, k, layouts[1], npdt)
        lx, ly, bs, ierr = F.PRIMME_INT(dx.ld), F.PRIMME_INT(dy.ld), C.c_int(k), C.c_int(-1)
        self.dev.lib.primme_amd_amg_precond(dx.ptr, C.byref(lx), dy.ptr, C.byref(ly), C.byref(bs), C.byref(self.p), C.byref(ierr))
        assert ierr.value == 0
        assert np.array_equal(dx.block(), dx.host)
        return dy.block().T

    def close(self):
        self.dev.lib.primme_amd_operator_destroy(self.op)
        self.dev.lib.hipk_csr_destroy(self.A)


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("name", ["lap_33x35", "lap_33x35_shift", "lap_9x8x7", "lunda_x4"])
def test_application_against_the_restatement(dev, name, dt):
    rp, ci, va, shift = _case(name)
    va = va.astype(NPDT[dt])                                       # the matrix the device has
    m = len(rp) - 1
    rc, lv, _ = SA.c_plan(dev.lib, rp, ci, va, shift=shift)
    assert rc == 0 and len(lv) >= 2
    rng = np.random.default_rng(m + dt)
    hi_t, lo_t = (np.longdouble, np.float64) if dt == F.HIPK_F64 else (np.float64, np.float32)
    H_hi, H_lo = SA.Hierarchy(lv, dt=hi_t), SA.Hierarchy(lv, dt=lo_t)
    op = _Op(dev, rp, ci, va, dt, shift=shift)
    try:
        assert op.rc == 0
        for k in (1, 11):
            x = rng.standard_normal((m, k)).astype(np.float32).astype(np.float64)       # the same block in every precision
            ref = H_hi.vcycle(x.astype(hi_t))
            own = float(np.abs(H_lo.vcycle(x.astype(lo_t)).astype(hi_t) - ref).max())
            dev.lib.primme_amd_amg_stats(None, None, None)
            got = op.apply(x, rng)
            ap, la, nl = C.c_long(0), C.c_long(0), C.c_long(0)
            dev.lib.primme_amd_amg_stats(C.byref(ap), C.byref(la), C.byref(nl))
            err = float(np.abs(got - ref.astype(np.float64)).max())
            print(f"{name} {NPDT[dt].__name__} {k} columns: levels {[v['n'] for v in lv]}, |device - reference| = {err:.3e}, the "
                  f"restatement's own rounding {own:.3e} (ratio {err / own:.2f}), |K^-1 x| = {float(np.abs(ref).max()):.3e}; {la.value} launches")
            assert err <= 64 * own
            # 11 launches per level but the last, as with plain aggregation; there the dense inverse in one; per chunk of 8 columns
            chunks = (k + 7) // 8
            assert (ap.value, la.value, nl.value) == (k, chunks * (11 * (len(lv) - 1) + 1), len(lv))
    finally:
        op.close()


def test_set_amg_smoothed_return_codes(dev):
    lib = dev.lib
    rp, ci, va = problems.laplacian_csr((6, 7))[:3]
    o = _Op(dev, rp, ci, va, F.HIPK_F64)
    assert o.rc == 0
    ptr = lambda a: a.ctypes.data_as(C.c_void_p)
    sa = lambda rp_=rp, ci_=ci, va_=va, nu=2, ncs=16, theta=0.08, omega=SA.OMEGA, shift=0.0, op=o.op: \
        lib.primme_amd_operator_set_amg_smoothed(op, ptr(rp_), ptr(ci_), ptr(va_), nu, ncs, theta, omega, shift)
    assert sa() == 0 and sa(nu=1, ncs=1, theta=0.0, omega=1.99, shift=3.0) == 0 and sa(omega=0.01) == 0
    assert sa(nu=0) == -1 and sa(ncs=0) == -1
    assert sa(theta=1.0) == -1 and sa(theta=-0.01) == -1 and sa(theta=float("nan")) == -1
    assert sa(omega=0.0) == -1 and sa(omega=2.0) == -1 and sa(omega=-1.0) == -1 and sa(omega=float("nan")) == -1
    assert sa(shift=-0.5) == -1 and sa(shift=float("nan")) == -1
    assert sa(op=None) == -1 and lib.primme_amd_operator_set_amg_smoothed(o.op, None, ptr(ci), ptr(va), 2, 16, 0.08, SA.OMEGA, 0.0) == -1
    rp2, ci2, va2 = problems.laplacian_csr((6, 8))[:3]
    assert sa(rp_=rp2, ci_=ci2, va_=va2) == -1                          # another pattern than the operator's
    vb = va.copy()
    vb[ci == np.repeat(np.arange(42), np.diff(rp))] = 0.0
    assert sa(va_=vb) == -1                                             # the plan refuses a diagonal of zeros
    vb[ci == np.repeat(np.arange(42), np.diff(rp))] = 0.5
    assert sa(va_=vb) == -1                                             # indefinite: the Cholesky factorisation fails
    assert lib.primme_amd_operator_set_complex(o.op, 1) == 0 and sa() == -44
    assert lib.primme_amd_operator_set_complex(o.op, 0) == 0 and sa() == 0
    o.close()
    A, op = C.c_void_p(), C.c_void_p()
    assert lib.hipk_stencil_create(dev.ctx, F.HIPK_F64, 6, 7, 1, 0, 42, C.byref(A)) == 0
    assert lib.primme_amd_operator_create(C.byref(op), A, None) == 0
    assert sa(op=op) == -44                                             # a stencil operator has the geometric multigrid
    lib.primme_amd_operator_destroy(op); lib.hipk_csr_destroy(A)


def test_a_plain_configuration_replaces_a_smoothed_one(dev):
    """set_amg after set_amg_smoothed on one operator: the cycle goes back to the aggregate kernels (and the other way round)"""
    rp, ci, va, shift = _case("lap_33x35")
    m = len(rp) - 1
    rng = np.random.default_rng(9)
    x = rng.standard_normal((m, 2)).astype(np.float32).astype(np.float64)
    rc, lv = AMG.c_plan(dev.lib, rp, ci, va)
    assert rc == 0
    rc, lvs, _ = SA.c_plan(dev.lib, rp, ci, va)
    assert rc == 0
    ref_plain, ref_smooth = AMG.Hierarchy(lv).vcycle(x), SA.Hierarchy(lvs).vcycle(x)
    assert np.abs(ref_plain - ref_smooth).max() > 1e-3 * np.abs(ref_plain).max()          # the two cycles differ
    # 1e-11: four orders above the rounding of a two-level cycle in double (the ratios of the test above), eight below the
    # difference of the two cycles
    op = _Op(dev, rp, ci, va, F.HIPK_F64)
    try:
        assert op.rc == 0
        assert np.abs(op.apply(x, rng) - ref_smooth).max() <= 1e-11 * np.abs(ref_smooth).max()
        assert dev.lib.primme_amd_operator_set_amg(op.op, *op.args, 2, 16, 0.08, 1.0, 0.0) == 0
        assert np.abs(op.apply(x, rng) - ref_plain).max() <= 1e-11 * np.abs(ref_plain).max()
        assert dev.lib.primme_amd_operator_set_amg_smoothed(op.op, *op.args, 2, 16, 0.08, SA.OMEGA, 0.0) == 0
        assert np.abs(op.apply(x, rng) - ref_smooth).max() <= 1e-11 * np.abs(ref_smooth).max()
    finally:
        op.close()
