"""The device pieces of the aggregation algebraic multigrid preconditioner (csrc/hipk_amg.hip, primme_amd_amg_precond in
csrc/amd_operator.hip) against numpy, at the smallest shapes that can go wrong.

hipk_amg_smooth_update, hipk_amg_restrict, hipk_amg_prolong_add: 1, 2, 63, 64, 65, 257, 1025 rows (below, at and above a wave,
across a workgroup's first trip), 1, 3 and 8 columns, double and float, three layouts: 16-byte aligned base and leading
dimension (the 16-byte accesses), an odd leading dimension and a base one element off (the element path).  The aggregate maps
are generated, in range, a random partition of the rows with every aggregate's rows ascending; one map mixes aggregates of 1, 2,
63, 64, 65 and 300 rows (at most 64: the lane's own sum, more: the wave's), shuffled so that the 2 or 4 aggregates of a lane
mix both kinds, and one has more aggregates than a workgroup takes in its two trips.  hipk_amg_dense_apply at n = 1, 2, 63,
64, 65, 256.  Panels are NaN outside the block, so an access outside shows.  Every output is a sum that the kernels accumulate
in double and round once to the panel type: per element |out - ref| <= 32 eps sum |terms|, eps of the panel type, ref and the
terms in float64 from the inputs as rounded to the panel type.  The restriction run twice is bit-identical.

The whole application K^-1 x on 33 x 35 (shift 0 and 0.5), 9 x 8 x 7 and LUNDA.mtx against the restatement of
tests/amg_cases.py on the library's own plan, 1 and 11 columns (a chunk of 8 and one of 3): the difference to the cycle in
longdouble is at most 64 x what the SAME cycle in float64 differs from it; in float the pair is float64 / float32.  The
counters, and the return codes of primme_amd_operator_set_amg."""
import ctypes as C

import numpy as np
import pytest

import amg_cases as AMG
from kernel_harness import Dev, NPDT
from primme_amd import _ffi as F
from primme_amd import problems

pytestmark = pytest.mark.gpu
DTYPES = [F.HIPK_F64, F.HIPK_F32]
EPS = {F.HIPK_F64: 2.0 ** -52, F.HIPK_F32: 2.0 ** -23}
ROWS = (1, 2, 63, 64, 65, 257, 1025)
NCOLS = (1, 3, 8)
LAYOUTS = ("aligned", "odd_ld", "base_off")
TINY = np.finfo(np.float64).tiny


@pytest.fixture(scope="module")
def dev(built):
    d = Dev()
    yield d
    d.close()


def _stream(dev):
    return C.c_void_p(dev.lib.hipk_ctx_stream(dev.ctx))


def _layout(m, layout):
    """(leading dimension, base offset in elements)"""
    if layout == "aligned":
        return (m + 3) // 4 * 4, 0
    if layout == "odd_ld":
        return (m + 1) | 1, 0
    return (m + 3) // 4 * 4 + 4, 1


class _Panel:
    """a device panel of nc columns of m rows, ld elements apart, starting `base` elements into its buffer; NaN everywhere else"""

    def __init__(self, dev, rng, m, nc, layout, npdt, fill=None):
        self.dev, self.m, self.nc = dev, m, nc
        self.ld, self.base = _layout(m, layout)
        h = np.full(self.base + (nc + 1) * self.ld, np.nan, dtype=npdt)
        v = h[self.base:self.base + nc * self.ld].reshape(nc, self.ld)
        v[:, :m] = rng.standard_normal((nc, m)) if fill is None else fill
        self.host = v[:, :m].astype(np.float64)
        self.t = dev.arr(h)
        self.ptr = dev.ptr(self.t, self.base)

    def block(self):
        """the block now on the device, after checking that nothing outside it was written"""
        h = self.dev.get(self.t)
        v = h[self.base:self.base + self.nc * self.ld].reshape(self.nc, self.ld)
        assert np.all(np.isnan(h[:self.base])) and np.all(np.isnan(h[self.base + self.nc * self.ld:])) and np.all(np.isnan(v[:, self.m:]))
        return v[:, :self.m].astype(np.float64)


def _ivec(dev, a):
    return dev.arr(np.ascontiguousarray(a, dtype=np.int32))


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("m", ROWS)
def test_smooth_update(dev, m, dt):
    npdt, lib = NPDT[dt], dev.lib
    rng = np.random.default_rng(m + dt)
    worst = 0.0
    dinv = 0.25 + rng.random(m)
    ddev = dev.arr(np.concatenate([[np.nan, np.nan], dinv, [np.nan]]))            # 16-byte aligned at element 2, not at 1 and 3
    ddev_off = dev.arr(np.concatenate([[np.nan], dinv, [np.nan]]))
    for nc in NCOLS:
        cf = F.HipkChebCoef()
        for c in range(8):
            cf.cy[c], cf.cp[c], cf.cx[c], cf.cw[c] = 1.1 + 0.1 * c, -0.6 - 0.05 * c, 0.8 + 0.03 * c, -0.45 + 0.02 * c
        col = lambda a: np.array(a[:nc])[:, None]
        for layout in LAYOUTS:
            dptr = dev.ptr(ddev_off, 1) if layout == "base_off" else dev.ptr(ddev, 2)
            for variant in ("apart", "out_on_yprev", "out_on_w", "no_w", "no_yk", "no_yprev", "residual"):
                x, w, yk, yp, o = (_Panel(dev, rng, m, nc, layout, npdt) for _ in range(5))
                has_w, has_k, has_p = variant != "no_w", variant not in ("no_yk", "residual"), variant not in ("no_yprev", "residual")
                has_d = variant != "residual"
                out = yp if variant == "out_on_yprev" else w if variant == "out_on_w" else o
                rc = lib.hipk_amg_smooth_update(_stream(dev), dt, m, nc, C.byref(cf), dptr if has_d else None, x.ptr, x.ld,
                                                w.ptr if has_w else None, w.ld, yk.ptr if has_k else None, yk.ld,
                                                yp.ptr if has_p else None, yp.ld, out.ptr, out.ld)
                assert rc == 0, (variant, nc, layout)
                d = dinv[None, :] if has_d else np.ones((1, m))
                ref, mag = d * col(cf.cx) * x.host, np.abs(d * col(cf.cx) * x.host)
                if has_w: ref, mag = ref + d * col(cf.cw) * w.host, mag + np.abs(d * col(cf.cw) * w.host)
                if has_k: ref, mag = ref + col(cf.cy) * yk.host, mag + np.abs(col(cf.cy) * yk.host)
                if has_p: ref, mag = ref + col(cf.cp) * yp.host, mag + np.abs(col(cf.cp) * yp.host)
                ratio = np.abs(out.block() - ref) / np.maximum(32 * EPS[dt] * mag, TINY)
                assert ratio.max() <= 1.0, (variant, nc, layout, float(ratio.max()))
                worst = max(worst, float(ratio.max()))
                for p in (x, w, yk, yp):                                  # the inputs are left alone
                    if p is not out:
                        assert np.array_equal(p.block(), p.host)
    print(f"smooth update {m} rows {npdt.__name__}: largest |out - ref| / (32 eps sum|terms|) = {worst:.3f}")


def _random_map(rng, sizes):
    """(agg, aggptr, aggrows, rows): the aggregates take a random partition of the rows, each one's rows ascending"""
    sizes = np.asarray(sizes)
    nf = int(sizes.sum())
    perm = rng.permutation(nf)
    aggptr = np.concatenate([[0], np.cumsum(sizes)])
    aggrows = np.concatenate([np.sort(perm[aggptr[j]:aggptr[j + 1]]) for j in range(len(sizes))])
    agg = np.empty(nf, dtype=np.int64)
    agg[aggrows] = np.repeat(np.arange(len(sizes)), sizes)
    return agg, aggptr, aggrows, nf


def _sizes_for_rows(rng, nf):
    """aggregate sizes 1 .. 9 that add up to nf"""
    s = []
    while sum(s) < nf:
        s.append(int(min(rng.integers(1, 10), nf - sum(s))))
    return s


def _mix(rng, filler):
    s = [1, 2, 63, 64, 65, 300] * 3 + [1] * filler + [3] * 50
    return [int(v) for v in rng.permutation(s)]


MAPS = [("rows", nf) for nf in ROWS] + [("mix", 600), ("mix", 2500), ("one", 300), ("one", 64), ("identity", 129)]


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("kind,arg", MAPS)
def test_restrict_and_prolong(dev, kind, arg, dt):
    npdt, lib = NPDT[dt], dev.lib
    rng = np.random.default_rng(arg + 7 * dt)
    sizes = {"rows": lambda: _sizes_for_rows(rng, arg), "mix": lambda: _mix(rng, arg), "one": lambda: [arg],
             "identity": lambda: [1] * arg}[kind]()
    agg, aggptr, aggrows, nf = _random_map(rng, sizes)
    ncg = len(sizes)
    dagg, dptr, drows = _ivec(dev, agg), _ivec(dev, aggptr), _ivec(dev, aggrows)
    worst = [0.0, 0.0]
    for nc in NCOLS:
        for layout in LAYOUTS:
            f = _Panel(dev, rng, nf, nc, layout, npdt)
            c = _Panel(dev, rng, ncg, nc, layout, npdt)
            assert lib.hipk_amg_restrict(_stream(dev), dt, nf, ncg, dev.ptr(dptr), dev.ptr(drows), nc, f.ptr, f.ld, c.ptr, c.ld) == 0
            got = c.block()
            ref, mag = np.zeros((nc, ncg)), np.zeros((nc, ncg))
            for k in range(nc):
                np.add.at(ref[k], agg, f.host[k])
                np.add.at(mag[k], agg, np.abs(f.host[k]))
            ratio = np.abs(got - ref) / np.maximum(32 * EPS[dt] * mag, TINY)
            assert ratio.max() <= 1.0, ("restrict", nc, layout, float(ratio.max()))
            worst[0] = max(worst[0], float(ratio.max()))
            assert np.array_equal(f.block(), f.host)
            # the same again: every sum has one order
            c2 = _Panel(dev, rng, ncg, nc, layout, npdt)
            assert lib.hipk_amg_restrict(_stream(dev), dt, nf, ncg, dev.ptr(dptr), dev.ptr(drows), nc, f.ptr, f.ld, c2.ptr, c2.ld) == 0
            assert np.array_equal(c2.block(), got)
            # Y += over C[agg]
            cc = _Panel(dev, rng, ncg, nc, layout, npdt)
            y = _Panel(dev, rng, nf, nc, layout, npdt)
            over = 1.0 if nc == 3 else 1.375
            assert lib.hipk_amg_prolong_add(_stream(dev), dt, nf, ncg, dev.ptr(dagg), over, nc, cc.ptr, cc.ld, y.ptr, y.ld) == 0
            ref = y.host + over * cc.host[:, agg]
            ratio = np.abs(y.block() - ref) / np.maximum(32 * EPS[dt] * (np.abs(y.host) + np.abs(over * cc.host[:, agg])), TINY)
            assert ratio.max() <= 1.0, ("prolong", nc, layout, float(ratio.max()))
            worst[1] = max(worst[1], float(ratio.max()))
            assert np.array_equal(cc.block(), cc.host)
    print(f"{kind} {arg}: {nf} rows -> {ncg} aggregates (largest {max(sizes)}) {npdt.__name__}: restrict {worst[0]:.3f}, prolong {worst[1]:.3f} of the bound")


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("n", [1, 2, 63, 64, 65, 256])
def test_dense_apply(dev, n, dt):
    npdt, lib = NPDT[dt], dev.lib
    rng = np.random.default_rng(n + 3 * dt)
    G = rng.standard_normal((n, n))
    G = G + G.T
    dG = dev.arr(G)
    worst = 0.0
    for nc in NCOLS:
        for layout in LAYOUTS:
            x = _Panel(dev, rng, n, nc, layout, npdt)
            y = _Panel(dev, rng, n, nc, layout, npdt)
            assert lib.hipk_amg_dense_apply(_stream(dev), dt, n, dev.ptr(dG), nc, x.ptr, x.ld, y.ptr, y.ld) == 0
            ratio = np.abs(y.block() - x.host @ G) / np.maximum(32 * EPS[dt] * (np.abs(x.host) @ np.abs(G)), TINY)
            assert ratio.max() <= 1.0, (nc, layout, float(ratio.max()))
            worst = max(worst, float(ratio.max()))
            assert np.array_equal(x.block(), x.host)
    print(f"dense apply n = {n} {npdt.__name__}: largest |out - ref| / (32 eps sum|terms|) = {worst:.3f}")


def test_kernel_argument_errors(dev):
    lib, st = dev.lib, _stream(dev)
    rng = np.random.default_rng(1)
    a, b = (_Panel(dev, rng, 12, 9, "aligned", np.float64) for _ in range(2))
    agg, aggptr, aggrows, nf = _random_map(rng, [3, 4, 5])
    dagg, dptr, drows = _ivec(dev, agg), _ivec(dev, aggptr), _ivec(dev, aggrows)
    G = dev.arr(np.eye(12))
    cf = F.HipkChebCoef()
    upd = lambda dt, m, nc, x, out: lib.hipk_amg_smooth_update(st, dt, m, nc, C.byref(cf), None, x, 12, None, 0, None, 0, None, 0, out, 12)
    res = lambda dt, nc, f, c: lib.hipk_amg_restrict(st, dt, 12, 3, dev.ptr(dptr), dev.ptr(drows), nc, f, 12, c, 12)
    pro = lambda dt, nc, c, y: lib.hipk_amg_prolong_add(st, dt, 12, 3, dev.ptr(dagg), 1.0, nc, c, 12, y, 12)
    den = lambda dt, n, nc, x, y: lib.hipk_amg_dense_apply(st, dt, n, dev.ptr(G), nc, x, 12, y, 12)
    for cdt in (F.HIPK_C64, F.HIPK_C32):
        assert upd(cdt, 12, 1, a.ptr, b.ptr) == -44 and res(cdt, 1, a.ptr, b.ptr) == -44
        assert pro(cdt, 1, b.ptr, a.ptr) == -44 and den(cdt, 12, 1, a.ptr, b.ptr) == -44
    dt = F.HIPK_F64
    assert upd(dt, 12, 9, a.ptr, b.ptr) == -1 and res(dt, 9, a.ptr, b.ptr) == -1 and pro(dt, 9, b.ptr, a.ptr) == -1     # 9 columns
    assert den(dt, 12, 9, a.ptr, b.ptr) == -1
    assert upd(dt, 12, 1, a.ptr, None) == -1 and res(dt, 1, a.ptr, None) == -1 and pro(dt, 1, b.ptr, None) == -1         # no output
    assert den(dt, 12, 1, a.ptr, None) == -1
    assert upd(dt, 12, 1, None, b.ptr) == -1 and res(dt, 1, None, b.ptr) == -1 and pro(dt, 1, None, a.ptr) == -1
    assert lib.hipk_amg_dense_apply(st, dt, 257, dev.ptr(G), 1, a.ptr, 300, b.ptr, 300) == -1                            # n = 257
    assert den(dt, 0, 1, a.ptr, b.ptr) == -1
    assert lib.hipk_amg_restrict(st, dt, 3, 12, dev.ptr(dptr), dev.ptr(drows), 1, a.ptr, 12, b.ptr, 12) == -1            # nc > nf
    assert lib.hipk_amg_restrict(st, dt, 12, 3, None, dev.ptr(drows), 1, a.ptr, 12, b.ptr, 12) == -1
    assert lib.hipk_amg_prolong_add(st, dt, 12, 3, None, 1.0, 1, b.ptr, 12, a.ptr, 12) == -1
    assert res(dt, 1, a.ptr, a.ptr) == -1 and pro(dt, 1, a.ptr, a.ptr) == -1
    assert np.array_equal(a.block(), a.host) and np.array_equal(b.block(), b.host)          # nothing was launched


# ---- the whole application ------------------------------------------------------------------------------------------
def _case(name):
    if name == "lunda":
        rp, ci, va = AMG.lunda()
        return rp, ci, va, 0.0
    dims, shift = {"lap_33x35": ((33, 35), 0.0), "lap_33x35_shift": ((33, 35), 0.5), "lap_9x8x7": ((9, 8, 7), 0.0)}[name]
    rp, ci, va, _ = problems.laplacian_csr(dims)
    return rp, ci, va, shift


class _Op:
    """a CSR operator with the preconditioner configured, and the callback's parameter block"""

    def __init__(self, dev, rp, ci, va, dt, nu=2, ncs=16, theta=0.08, over=1.0, shift=0.0):
        self.dev, lib = dev, dev.lib
        self.m, self.dt = len(rp) - 1, dt
        rp, ci, va = np.ascontiguousarray(rp, dtype=np.int32), np.ascontiguousarray(ci, dtype=np.int32), np.ascontiguousarray(va, dtype=NPDT[dt])
        self.A, self.op = C.c_void_p(), C.c_void_p()
        args = (rp.ctypes.data_as(C.c_void_p), ci.ctypes.data_as(C.c_void_p), va.ctypes.data_as(C.c_void_p))
        assert lib.hipk_csr_create(dev.ctx, dt, self.m, self.m, 0, *args, C.byref(self.A)) == 0
        assert lib.primme_amd_operator_create(C.byref(self.op), self.A, None) == 0
        self.rc = lib.primme_amd_operator_set_amg(self.op, *args, nu, ncs, theta, over, shift)
        self.p = F.PrimmeParams()
        self.p.preconditioner = self.op

    def apply(self, x, rng, layouts=("odd_ld", "aligned")):
        """K^-1 x for a host block x [m, k] -> [m, k]"""
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
@pytest.mark.parametrize("name", ["lap_33x35", "lap_33x35_shift", "lap_9x8x7", "lunda"])
def test_application_against_the_restatement(dev, name, dt):
    rp, ci, va, shift = _case(name)
    va = va.astype(NPDT[dt])                                       # the matrix the device has
    m = len(rp) - 1
    rc, lv = AMG.c_plan(dev.lib, rp, ci, va, shift=shift)
    assert rc == 0
    rng = np.random.default_rng(m + dt)
    over = 1.25 if name == "lap_9x8x7" else 1.0
    hi_t, lo_t = (np.longdouble, np.float64) if dt == F.HIPK_F64 else (np.float64, np.float32)
    H_hi, H_lo = AMG.Hierarchy(lv, over=over, dt=hi_t), AMG.Hierarchy(lv, over=over, dt=lo_t)
    op = _Op(dev, rp, ci, va, dt, over=over, shift=shift)
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
            # V(2, 2): 11 launches per level but the last (4 products, 5 updates, restriction, interpolation); there the dense
            # inverse in one; per chunk of 8 columns
            chunks = (k + 7) // 8
            assert (ap.value, la.value, nl.value) == (k, chunks * (11 * (len(lv) - 1) + 1), len(lv))
    finally:
        op.close()


@pytest.mark.parametrize("dt", DTYPES)
def test_chebyshev_last_level_and_other_step_counts(dev, dt):
    """a last level above 256 rows (a diagonal matrix stalls at once; 300 blocks of the 1-D Laplacian of 4 rows stall after two
    levels, one row per block) and V(3, 3) / V(1, 1): the panel bookkeeping for odd and single step counts"""
    rng = np.random.default_rng(5 + dt)
    hi_t, lo_t = (np.longdouble, np.float64) if dt == F.HIPK_F64 else (np.float64, np.float32)
    cases = [(AMG.matrices()["diag_300"], dict(nu=2, ncs=5)), (AMG.matrices()["diag_300"], dict(nu=2, ncs=1))]
    rp, ci, va = problems.laplacian_csr((33, 35))[:3]
    cases += [((rp, ci, va), dict(nu=3, ncs=2, shift=0.25, over=1.5)), ((rp, ci, va), dict(nu=1, ncs=1))]
    blocks = problems.tile_block_diagonal(*problems.laplacian_csr((4,))[:3], 300, scale_fn=lambda t: 1.0 + 0.01 * t)
    cases += [(blocks, dict(nu=2, ncs=4, shift=0.125))]
    for (rp, ci, va), kw in cases:
        va = np.asarray(va, dtype=np.float64).astype(NPDT[dt])
        m = len(rp) - 1
        rc, lv = AMG.c_plan(dev.lib, rp, ci, va, shift=kw.get("shift", 0.0), theta=kw.get("theta", 0.08))
        assert rc == 0
        H = [AMG.Hierarchy(lv, kw["nu"], kw["ncs"], kw.get("over", 1.0), dt=t) for t in (hi_t, lo_t)]
        x = rng.standard_normal((m, 3)).astype(np.float32).astype(np.float64)
        ref = H[0].vcycle(x.astype(hi_t))
        own = float(np.abs(H[1].vcycle(x.astype(lo_t)).astype(hi_t) - ref).max())
        op = _Op(dev, rp, ci, va, dt, **kw)
        try:
            assert op.rc == 0
            dev.lib.primme_amd_amg_stats(None, None, None)
            got = op.apply(x, rng, layouts=("aligned", "base_off"))
            ap, la, nl = C.c_long(0), C.c_long(0), C.c_long(0)
            dev.lib.primme_amd_amg_stats(C.byref(ap), C.byref(la), C.byref(nl))
        finally:
            op.close()
        err = float(np.abs(got - ref.astype(np.float64)).max())
        last = 1 if lv[-1]["n"] <= AMG.DENSE_ROWS else 2 * kw["ncs"] - 1
        print(f"levels {[v['n'] for v in lv]} {kw} {NPDT[dt].__name__}: |device - reference| = {err:.3e}, own rounding {own:.3e}; {la.value} launches")
        assert err <= 64 * own
        assert (ap.value, la.value, nl.value) == (3, (4 * kw["nu"] + 3) * (len(lv) - 1) + last, len(lv))


def test_set_amg_return_codes(dev):
    lib = dev.lib
    lib.primme_amd_amg_stats(None, None, None)
    rp, ci, va = problems.laplacian_csr((6, 7))[:3]
    o = _Op(dev, rp, ci, va, F.HIPK_F64)
    assert o.rc == 0
    ptr = lambda a: a.ctypes.data_as(C.c_void_p)
    sa = lambda rp_=rp, ci_=ci, va_=va, nu=2, ncs=16, theta=0.08, over=1.0, shift=0.0, op=o.op: lib.primme_amd_operator_set_amg(
        op, ptr(rp_), ptr(ci_), ptr(va_), nu, ncs, theta, over, shift)
    assert sa() == 0 and sa(nu=1, ncs=1, theta=0.0, over=1.99, shift=3.0) == 0
    assert sa(nu=0) == -1 and sa(ncs=0) == -1
    assert sa(theta=1.0) == -1 and sa(theta=-0.01) == -1 and sa(theta=float("nan")) == -1
    assert sa(over=0.99) == -1 and sa(over=2.0) == -1 and sa(over=float("nan")) == -1
    assert sa(shift=-0.5) == -1 and sa(shift=float("nan")) == -1
    assert sa(op=None) == -1 and lib.primme_amd_operator_set_amg(o.op, None, ptr(ci), ptr(va), 2, 16, 0.08, 1.0, 0.0) == -1
    rp2, ci2, va2 = problems.laplacian_csr((6, 8))[:3]
    assert sa(rp_=rp2, ci_=ci2, va_=va2) == -1                          # another pattern than the operator's
    vb = va.copy()
    vb[ci == np.repeat(np.arange(42), np.diff(rp))] = 0.0
    assert sa(va_=vb) == -1                                             # the plan refuses a diagonal of zeros
    vb[ci == np.repeat(np.arange(42), np.diff(rp))] = 0.5
    assert sa(va_=vb) == -1                                             # indefinite: the Cholesky factorisation fails
    # the real-equivalent mode of a Hermitian problem
    assert lib.primme_amd_operator_set_complex(o.op, 1) == 0 and sa() == -44
    assert lib.primme_amd_operator_set_complex(o.op, 0) == 0 and sa() == 0
    o.close()
    A, op = C.c_void_p(), C.c_void_p()
    assert lib.hipk_stencil_create(dev.ctx, F.HIPK_F64, 6, 7, 1, 0, 42, C.byref(A)) == 0
    assert lib.primme_amd_operator_create(C.byref(op), A, None) == 0
    assert sa(op=op) == -44                                             # a stencil operator has the geometric multigrid
    lib.primme_amd_operator_destroy(op); lib.hipk_csr_destroy(A)
    vz = va.astype(np.complex128)
    assert lib.hipk_csr_create(dev.ctx, F.HIPK_C64, 42, 42, 0, ptr(rp), ptr(ci), ptr(vz), C.byref(A)) == 0
    assert lib.primme_amd_operator_create(C.byref(op), A, None) == 0
    assert sa(op=op) == -44                                             # a complex operator
    lib.primme_amd_operator_destroy(op); lib.hipk_csr_destroy(A)
    ap, la, nl = C.c_long(-1), C.c_long(-1), C.c_long(-1)
    lib.primme_amd_amg_stats(C.byref(ap), C.byref(la), C.byref(nl))
    assert (ap.value, la.value, nl.value) == (0, 0, 0)                  # nothing was launched
