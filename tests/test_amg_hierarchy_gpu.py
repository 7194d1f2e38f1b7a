"""The reusable hierarchy on the MI355X: primme_amd.AmgHierarchy and precond=("amg_hierarchy", H, ...) (primme_amd/api.py ->
primme_amd_amg_hierarchy_create, primme_amd_operator_set_amg_hierarchy).

setup="host", smoothed and plain: evals, resNorms, outer iterations and the AMG statistics of a solve are those of
("amg_smoothed",) / ("amg",) bit for bit, on 33 x 35 and on the four tiles of LUNDA.mtx.
setup="device": the downloaded plan level by level against the host's stages and the numpy restatement run on the level the
device has (tests/amg_hierarchy_cases.py: the aggregates and the indices equal, P and R the same bits, M_{l+1} within 32 eps
sum|terms|, exactly symmetric): level 0 is the host plan's; from level 1 on M_l differs from the host plan's in rounding and the
aggregation breaks ties between equal couplings by the last bit (65 x 67: M_2 has 1634 entries against the host plan's 1640 in
the same 120 rows), so the host's stages are run on the downloaded M_l.  The levels [1155, 206] and [4355, 748, 120] of 4p; one application K b of 1 and 11 columns within 64 x the
same-precision restatement's own rounding of the longdouble restatement on the downloaded plan; the 33 x 35 solve against the
analytic eigenvalues in fewer outer iterations than plain aggregation's 121 (the count is printed: the device plan differs from
the host's in rounding).  Reuse: two solves on one H, set up once, the second equal to a solve on a fresh H.  Lifetime: either
side closed first, a float32 session after a float64 one, an operator of another size, the device set-up of plain aggregation,
and a lowered entry limit that sends every level to the host routines: then the host plan bit for bit."""
import ctypes as C
import os

import numpy as np
import pytest

import amg_cases as AMG
import amg_hierarchy_cases as HC
import amg_smoothed_cases as SA
import primme_amd
from checkers import Operator, Session
from kernel_harness import Dev, NPDT
from primme_amd import _ffi as F
from primme_amd import problems
from primme_amd.api import amg_download_plan
from test_amg_kernels_gpu import _Panel

LIMIT = "PRIMME_AMD_AMG_SETUP_MAX_ENTRIES"

pytestmark = pytest.mark.gpu
KW = dict(numEvals=6, method="GD_plusK", eps=1e-10, aNorm=8.0)


def _matrix(name):
    if name == "lunda_x4":
        return tuple(AMG.lunda_tiled(4))
    return problems.laplacian_csr({"lap_33x35": (33, 35), "lap_65x67": (65, 67)}[name])[:3]


def _same_solve(a, b):
    assert a.ret == 0 and b.ret == 0
    assert np.array_equal(a.evals.view(np.int64), b.evals.view(np.int64)) and np.array_equal(a.resNorms.view(np.int64), b.resNorms.view(np.int64))
    assert a.stats["numOuterIterations"] == b.stats["numOuterIterations"] and a.stats["numMatvecs"] == b.stats["numMatvecs"]
    assert a.precond_stats == b.precond_stats


@pytest.mark.parametrize("smoothed", [True, False])
@pytest.mark.parametrize("name", ["lap_33x35", "lunda_x4"])
def test_host_setup_is_the_tuple_preconditioner(built, name, smoothed):
    rp, ci, va = _matrix(name)
    n = len(rp) - 1
    kw = dict(KW, v0=problems.start_vector(n), aNorm=float(np.abs(va).max() * 8))
    s = Session(Operator(n, csr=(rp, ci, va)), backend="hip")
    try:
        ref = s.solve(precond=("amg_smoothed",) if smoothed else ("amg",), **kw)
        with primme_amd.AmgHierarchy(s, smoothed=smoothed, setup="host") as H:
            got = s.solve(precond=("amg_hierarchy", H), **kw)
            assert H.times_attached == 1 and H.fallback_levels == 0 and H.device_seconds == 0.0 and H.levels == got.precond_stats["levels"]
        _same_solve(got, ref)
        print(f"{name} {'smoothed' if smoothed else 'plain'}: {got.stats['numOuterIterations']} outer iterations either way, {got.precond_stats}")
    finally:
        s.close()


def _check_plan(plan, rp, ci, va, host, omega=SA.OMEGA):
    """the downloaded plan of a device set-up, level by level"""
    assert [v["n"] for v in plan] == [v["n"] for v in host]
    lv0 = dict(plan[0], rowptr=np.asarray(rp, dtype=np.int64), colind=np.asarray(ci, dtype=np.int64), values=np.asarray(va, dtype=np.float64))
    levels = [lv0] + plan[1:]
    worst = 0.0
    for l in range(len(levels) - 1):
        v = levels[l]
        if l == 0:
            hl = host
        else:
            # M_l differs from the host plan's in rounding, and the aggregation breaks ties between equal couplings by the last
            # bit: from level 1 on the host's stages are run on the level the device has (the host plan of M_l is its level 0)
            rc, hl, _ = SA.c_plan(F.load_product(), v["rowptr"], v["colind"], v["values"], omega=omega)
            assert rc == 0 and len(hl) >= 2 and HC.same_bits(hl[0]["dinv"], v["dinv"]) and hl[0]["rho"] == v["rho"]
        for k in ("agg", "aggptr", "aggrows", "prowptr", "pcolind", "rrowptr", "rcolind"):
            assert np.array_equal(v[k], hl[0][k]), (l, k)
        ref = HC.level(v["rowptr"], v["colind"], v["values"], v["dinv"], v["rho"], v["agg"], v["nc"], omega)
        worst = max(worst, HC.check_level(HC.host_level(v, levels[l + 1]), ref, HC.host_level(hl[0], hl[1])))
        rdinv, rrho = HC.finish(levels[l + 1]["rowptr"], levels[l + 1]["colind"], levels[l + 1]["values"])
        assert np.abs(levels[l + 1]["dinv"] - rdinv).max() <= 2 * HC.EPS * np.abs(rdinv).max() and abs(levels[l + 1]["rho"] - rrho) <= 4 * HC.EPS * rrho
    assert "prowptr" not in levels[-1] and levels[-1]["nc"] == 0
    return levels, worst


@pytest.mark.parametrize("name,rows", [("lap_33x35", [1155, 206]), ("lap_65x67", [4355, 748, 120]), ("lunda_x4", [588, 64])])
def test_device_setup_plan(built, name, rows):
    rp, ci, va = _matrix(name)
    n = len(rp) - 1
    lib = F.load_product()
    rc, host, _ = SA.c_plan(lib, rp, ci, va)
    assert rc == 0
    s = Session(Operator(n, csr=(rp, ci, va)), backend="hip")
    try:
        with primme_amd.AmgHierarchy(s) as H:
            assert H.rows == rows and H.levels == len(rows) and H.fallback_levels == 0 and 0.0 < H.device_seconds <= H.setup_seconds
            assert H.nnz[:2] == [v["nnz"] for v in host[:2]] and len(H.stage_seconds) == len(rows) - 1
            plan = H.plan()
            _, worst = _check_plan(plan, rp, ci, va, host)
            print(f"{name}: levels {H.rows}, set-up {H.setup_seconds:.4f} s ({H.device_seconds:.4f} s in the device stages), largest fraction of the "
                  f"bound on M_l {worst:.4f}; stages of level 0 {H.stage_seconds[0]}")
            with primme_amd.AmgHierarchy(s) as H2:                    # twice the same bits
                again = H2.plan()
            for a, b in zip(plan, again):
                assert a.keys() == b.keys()
                for k in a:
                    assert np.array_equal(np.asarray(a[k]), np.asarray(b[k])), k
        # every level sent to the host routines: the host plan bit for bit
        old = os.environ.get(LIMIT)
        try:
            os.environ[LIMIT] = "0"                                   # the C library reads the process environment at create
            with primme_amd.AmgHierarchy(s) as H3:
                assert H3.fallback_levels == len(rows) - 1 and H3.rows == rows
                fb = H3.plan()
        finally:
            if old is None:
                del os.environ[LIMIT]
            else:
                os.environ[LIMIT] = old
        for l, (a, b) in enumerate(zip(fb, host)):
            for k in a:
                if k not in ("rowptr", "colind", "values") or l > 0:
                    assert np.array_equal(np.asarray(a[k]), np.asarray(b[k])), (l, k)
    finally:
        s.close()


@pytest.mark.parametrize("dt", [F.HIPK_F64, F.HIPK_F32])
@pytest.mark.parametrize("name,shift", [("lap_33x35", 0.0), ("lap_33x35", 0.5), ("lunda_x4", 0.0)])
def test_device_setup_application(built, name, shift, dt):
    rp, ci, va = _matrix(name)
    m = len(rp) - 1
    dev = Dev()
    lib = dev.lib
    rp32, ci32, vat = np.ascontiguousarray(rp, dtype=np.int32), np.ascontiguousarray(ci, dtype=np.int32), np.ascontiguousarray(va, dtype=NPDT[dt])
    args = tuple(a.ctypes.data_as(C.c_void_p) for a in (rp32, ci32, vat))
    A, op, h = C.c_void_p(), C.c_void_p(), C.c_void_p()
    assert lib.hipk_csr_create(dev.ctx, dt, m, m, 0, *args, C.byref(A)) == 0 and lib.primme_amd_operator_create(C.byref(op), A, None) == 0
    try:
        assert lib.primme_amd_amg_hierarchy_create(op, *args, 1, 0.08, SA.OMEGA, shift, 1, C.byref(h)) == 0
        assert lib.primme_amd_operator_set_amg_hierarchy(op, h, 2, 16, 1.5) == -1                  # over with a smoothed hierarchy
        assert lib.primme_amd_operator_set_amg_hierarchy(op, h, 2, 16, 1.0) == 0
        rc, host, _ = SA.c_plan(lib, rp, ci, vat, shift=shift)
        assert rc == 0
        vs = vat.astype(np.float64)
        vs[ci == np.repeat(np.arange(m), np.diff(rp))] += shift
        levels, _ = _check_plan(amg_download_plan(lib, h), rp, ci, vs, host)
        for v in levels:
            v.setdefault("nnz", len(v["colind"]))
        nl = levels[-1]["n"]
        if nl <= AMG.DENSE_ROWS:
            levels[-1]["G"] = None                                     # the restatement inverts the last level itself
        hi_t, lo_t = (np.longdouble, np.float64) if dt == F.HIPK_F64 else (np.float64, np.float32)
        H_hi, H_lo = SA.Hierarchy(levels, dt=hi_t), SA.Hierarchy(levels, dt=lo_t)
        p = F.PrimmeParams()
        p.preconditioner = op
        rng = np.random.default_rng(m + dt)
        for k in (1, 11):
            x = rng.standard_normal((m, k)).astype(np.float32).astype(np.float64)
            ref = H_hi.vcycle(x.astype(hi_t))
            own = float(np.abs(H_lo.vcycle(x.astype(lo_t)).astype(hi_t) - ref).max())
            dx = _Panel(dev, rng, m, k, "odd_ld", NPDT[dt], fill=x.T)
            dy = _Panel(dev, rng, m, k, "aligned", NPDT[dt])
            lx, ly, bs, ierr = F.PRIMME_INT(dx.ld), F.PRIMME_INT(dy.ld), C.c_int(k), C.c_int(-1)
            lib.primme_amd_amg_precond(dx.ptr, C.byref(lx), dy.ptr, C.byref(ly), C.byref(bs), C.byref(p), C.byref(ierr))
            assert ierr.value == 0
            err = float(np.abs(dy.block().T - ref.astype(np.float64)).max())
            print(f"{name} shift {shift} {NPDT[dt].__name__} {k} columns: |device - reference| = {err:.3e}, the restatement's own rounding {own:.3e} "
                  f"(ratio {err / own:.2f})")
            assert err <= 64 * own
    finally:
        lib.primme_amd_amg_hierarchy_destroy(h)
        lib.primme_amd_operator_destroy(op)
        lib.hipk_csr_destroy(A)
        dev.close()


def test_device_setup_solve_and_reuse(built):
    rp, ci, va = _matrix("lap_33x35")
    n = len(rp) - 1
    kw = dict(KW, v0=problems.start_vector(n))
    exact = problems.laplacian_eigenvalues((33, 35), 6)
    s = Session(Operator(n, csr=(rp, ci, va)), backend="hip")
    try:
        H = primme_amd.AmgHierarchy(s)
        setup = H.setup_seconds
        first = s.solve(precond=("amg_hierarchy", H), **kw)
        assert first.ret == 0 and np.max(np.abs(first.evals - exact)) <= 1e-9 * 8.0 and np.all(first.resNorms <= 1e-10 * 8.0)
        its = first.stats["numOuterIterations"]
        print(f"33 x 35, device set-up: {its} outer iterations (host plan: 75, plain aggregation: 121), {first.precond_stats}")
        assert its < 121 and first.precond_stats["levels"] == 2 and first.precond_stats["applies"] == first.stats["numPreconds"] > 0
        second = s.solve(precond=("amg_hierarchy", H), **dict(kw, numEvals=3))
        assert H.times_attached == 2 and H.setup_seconds == setup
        with primme_amd.AmgHierarchy(s) as fresh:
            _same_solve(second, s.solve(precond=("amg_hierarchy", fresh), **dict(kw, numEvals=3)))
        # the smoother belongs to the attachment: V(1,1) on the same hierarchy converges too, with fewer launches per vector
        v11 = s.solve(precond=("amg_hierarchy", H, 1, 16), **kw)
        assert v11.ret == 0 and np.max(np.abs(v11.evals - exact)) <= 1e-9 * 8.0
        assert v11.precond_stats["launches"] / v11.precond_stats["applies"] < first.precond_stats["launches"] / first.precond_stats["applies"]
        H.close()
    finally:
        s.close()


def test_lifetime(built):
    rp, ci, va = _matrix("lap_33x35")
    n = len(rp) - 1
    op = Operator(n, csr=(rp, ci, va))
    kw = dict(KW, v0=problems.start_vector(n), numEvals=2)
    # the session first
    s = Session(op, backend="hip")
    H = primme_amd.AmgHierarchy(s)
    r64 = s.solve(precond=("amg_hierarchy", H), **kw)
    s.close()
    assert H.levels == 2 and H.times_attached == 1
    # a float32 session after the float64 one, on the same hierarchy
    s32 = Session(op, backend="hip", dtype=np.float32)
    r32 = s32.solve(precond=("amg_hierarchy", H), **dict(kw, eps=2e-6))
    assert r32.ret == 0 and np.abs(r32.evals - r64.evals).max() <= 1e-4 and H.times_attached == 2
    # the hierarchy first: the session keeps it alive
    H.close()
    again = s32.solve(precond=("amg_smoothed",), **dict(kw, eps=2e-6))         # and set_amg* releases it
    assert again.ret == 0
    s32.close()
    # an operator of another size; the device set-up of plain aggregation
    rp2, ci2, va2, n2 = problems.laplacian_csr((6, 8))
    s2, s3 = Session(Operator(n2, csr=(rp2, ci2, va2)), backend="hip"), Session(op, backend="hip")
    try:
        H3 = primme_amd.AmgHierarchy(s3, setup="host")
        with pytest.raises(ValueError, match="1155 rows"):
            s2.solve(precond=("amg_hierarchy", H3), **dict(KW, numEvals=2))
        lib = s2.lib
        assert lib.primme_amd_operator_set_amg_hierarchy(s2.oph, H3._h, 2, 16, 1.0) == -1
        assert lib.primme_amd_operator_set_amg_hierarchy(s3.oph, H3._h, 2, 16, 1.0) == 0
        assert lib.primme_amd_operator_set_amg_hierarchy(s3.oph, H3._h, 2, 16, 1.0) == 0          # itself again
        assert H3.times_attached == 2
        h = C.c_void_p()
        a = tuple(np.ascontiguousarray(x, dtype=t).ctypes.data_as(C.c_void_p) for x, t in ((rp, np.int32), (ci, np.int32), (va, np.float64)))
        assert lib.primme_amd_amg_hierarchy_create(s3.oph, *a, 0, 0.08, 0.0, 0.0, 1, C.byref(h)) == -44 and not h.value
        assert lib.primme_amd_amg_hierarchy_create(s3.oph, *a, 1, 0.08, 2.0, 0.0, 1, C.byref(h)) == -1
        assert lib.primme_amd_amg_hierarchy_create(None, *a, 1, 0.08, 1.0, 0.0, 1, C.byref(h)) == -1
        assert lib.primme_amd_amg_hierarchy_create(s3.oph, *a, 1, 0.08, 1.0, 0.0, -1, C.byref(h)) == -1 and not h.value
        assert lib.primme_amd_amg_hierarchy_create(s3.oph, *a, 1, 0.08, 1.0, 0.0, 2, C.byref(h)) == -1 and not h.value
        H3.close()
    finally:
        s2.close(); s3.close()
