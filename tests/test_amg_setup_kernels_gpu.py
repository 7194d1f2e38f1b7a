"""The four set-up kernels of csrc/hipk_amg_setup.hip, each on its own: hipk_amg_build_prolongation, hipk_amg_csr_transpose,
hipk_amg_galerkin and hipk_amg_level_finish, fed with the arrays of the host plan (primme_amd_amg_plan_create_smoothed) level by
level on the matrices of tests/amg_hierarchy_cases.py and omega in {4/3, 0.5}, and with aggregates of the test's own on the
matrices whose plan has one level (n = 1, n = 2, the diagonal matrix with its rows without an off-diagonal entry, the arrow
matrix whose row 0 has 300 entries in 150 aggregates).

Against the host plan and the numpy restatement: the indices of P, R and C equal, the values of P and R the same bits, C within
32 eps sum|terms| per entry and exactly symmetric, dinv within 2 eps, rho within 4 eps rho; a second run gives the same bits.
The flag of hipk_amg_level_finish on a zeroed, a negative and a missing diagonal entry; the entry limit that sends a level to
the host; the argument errors."""
import ctypes as C

import numpy as np
import pytest

import amg_hierarchy_cases as HC
import amg_smoothed_cases as SA
from kernel_harness import Dev, DevArray
from primme_amd import _ffi as F

pytestmark = pytest.mark.gpu
_mats = HC.matrices()
_PLAN_CASES = [n for n in _mats if n not in ("lap1d_1", "lap1d_2", "lap_6x7", "diag_300")]      # the others have one level


@pytest.fixture(scope="module")
def dev(built):
    d = Dev()
    yield d
    d.close()


def _st(dev):
    return C.c_void_p(dev.lib.hipk_ctx_stream(dev.ctx))


def _up(dev, rp, ci, va):
    return dev.arr(np.asarray(rp, dtype=np.int32)), dev.arr(np.asarray(ci, dtype=np.int32)), dev.arr(np.asarray(va, dtype=np.float64))


def _take(dev, ptrs, n1, nnz):
    """the three arrays a stage allocated, as numpy arrays; the device arrays are released"""
    out = (dev.get(DevArray(ptrs[0].value, (n1,), np.int32)).astype(np.int64), dev.get(DevArray(ptrs[1].value, (nnz,), np.int32)).astype(np.int64),
           dev.get(DevArray(ptrs[2].value, (nnz,), np.float64)))
    for p in ptrs:
        dev.lib.hipk_amg_setup_free(p)
    return out


def device_level(dev, rp, ci, va, dinv, rho, agg, nc, omega):
    """P, R, C, dinv and rho of C from the four kernels"""
    lib, st, n = dev.lib, _st(dev), len(rp) - 1
    M = _up(dev, rp, ci, va)
    ddinv, dagg = dev.arr(np.asarray(dinv, dtype=np.float64)), dev.arr(np.asarray(agg, dtype=np.int32))
    p, r, c = ([C.c_void_p() for _ in range(3)] for _ in range(3))
    pnnz, cnnz = C.c_int64(-1), C.c_int64(-1)
    assert lib.hipk_amg_build_prolongation(st, n, nc, *(dev.ptr(a) for a in M), dev.ptr(ddinv), dev.ptr(dagg), omega / rho, -1,
                                           *(C.byref(x) for x in p), C.byref(pnnz)) == 0
    assert lib.hipk_amg_csr_transpose(st, n, nc, pnnz.value, *p, -1, *(C.byref(x) for x in r)) == 0
    assert lib.hipk_amg_galerkin(st, n, nc, *(dev.ptr(a) for a in M), *p, *r, -1, *(C.byref(x) for x in c), C.byref(cnnz)) == 0
    cdinv, cdiag = dev.arr(np.full(nc, np.nan)), dev.arr(np.full(nc, np.nan))
    crho, flag = C.c_double(-1.0), C.c_int(-1)
    assert lib.hipk_amg_level_finish(st, nc, *c, dev.ptr(cdinv), dev.ptr(cdiag), C.byref(crho), C.byref(flag)) == 0
    out = dict(P=_take(dev, p, n + 1, pnnz.value), R=_take(dev, r, nc + 1, pnnz.value), C=_take(dev, c, nc + 1, cnnz.value),
               dinv=dev.get(cdinv), diag=dev.get(cdiag), rho=crho.value, flag=flag.value)
    assert out["P"][0][-1] == pnnz.value and out["R"][0][-1] == pnnz.value and out["C"][0][-1] == cnnz.value
    return out


def _check(dev, rp, ci, va, dinv, rho, agg, nc, omega, host=None):
    ref = HC.level(rp, ci, va, dinv, rho, agg, nc, omega)
    got = device_level(dev, rp, ci, va, dinv, rho, agg, nc, omega)
    worst = HC.check_level(got, ref, host)
    # dinv and rho of the coarse matrix the device built
    rdinv, rrho = HC.finish(*got["C"])
    assert got["flag"] == 0 and np.abs(got["dinv"] - rdinv).max() <= 2 * HC.EPS * np.abs(rdinv).max()
    assert np.abs(got["dinv"] * got["diag"] - 1.0).max() <= 2 * HC.EPS and abs(got["rho"] - rrho) <= 4 * HC.EPS * rrho
    again = device_level(dev, rp, ci, va, dinv, rho, agg, nc, omega)
    for k in ("P", "R", "C"):
        assert np.array_equal(again[k][0], got[k][0]) and np.array_equal(again[k][1], got[k][1]) and HC.same_bits(again[k][2], got[k][2]), k
    assert HC.same_bits(again["dinv"], got["dinv"]) and again["rho"] == got["rho"]
    return worst, got


@pytest.mark.parametrize("omega", HC.OMEGAS)
@pytest.mark.parametrize("name", _PLAN_CASES)
def test_kernels_against_the_host_plan(dev, name, omega):
    rp, ci, va, shift, theta = _mats[name]
    rc, lv, _ = SA.c_plan(dev.lib, rp, ci, va, shift=shift, theta=theta, omega=omega)
    assert rc == 0 and len(lv) >= 2
    worst = 0.0
    for l in range(len(lv) - 1):
        v = lv[l]
        w, got = _check(dev, v["rowptr"], v["colind"], v["values"], v["dinv"], v["rho"], v["agg"], v["nc"], omega, HC.host_level(v, lv[l + 1]))
        worst = max(worst, w)
    print(f"{name} omega {omega:.3f}: levels {[v['n'] for v in lv]}, longest row of R {[int(np.diff(v['rrowptr']).max()) for v in lv[:-1]]}, "
          f"largest |C - C_ref| / (32 eps sum|terms|) = {worst:.4f}")


@pytest.mark.parametrize("name", list(HC.custom_cases()))
def test_kernels_on_the_custom_aggregates(dev, name):
    rp, ci, va, agg = HC.custom_cases()[name]
    dinv, rho = HC.finish(rp, ci, va)
    worst, got = _check(dev, rp, ci, va, dinv, rho, agg, int(agg.max()) + 1, 4.0 / 3.0)
    print(f"{name}: P {len(got['P'][1])} entries, longest row of M {int(np.diff(rp).max())}, of R {int(np.diff(got['R'][0]).max())}, "
          f"C {len(got['C'][1])} entries, fraction of the bound {worst:.4f}")


def test_level_finish_on_the_matrices_and_the_flag(dev):
    lib, st = dev.lib, _st(dev)

    def run(rp, ci, va):
        n = len(rp) - 1
        M = _up(dev, rp, ci, va)
        dinv, diag = dev.arr(np.full(n, np.nan)), dev.arr(np.full(n, np.nan))
        rho, flag = C.c_double(-1.0), C.c_int(-1)
        assert lib.hipk_amg_level_finish(st, n, *(dev.ptr(a) for a in M), dev.ptr(dinv), dev.ptr(diag), C.byref(rho), C.byref(flag)) == 0
        return dev.get(dinv), dev.get(diag), rho.value, flag.value

    for name, (rp, ci, va, shift, theta) in _mats.items():
        rdinv, rrho = HC.finish(rp, ci, va)
        dinv, diag, rho, flag = run(rp, ci, va)
        assert flag == 0 and HC.same_bits(dinv, rdinv) and abs(rho - rrho) <= 4 * HC.EPS * rrho, name
        assert np.array_equal(diag, 1.0 / rdinv) or np.abs(diag * rdinv - 1).max() <= 2 * HC.EPS
    rp, ci, va = _mats["lap_33x35"][:3]
    d = np.flatnonzero(ci == np.repeat(np.arange(len(rp) - 1), np.diff(rp)))
    for bad in (0.0, -4.0):
        vb = va.copy()
        vb[d[700]] = bad
        assert run(rp, ci, vb)[3] == 1
    keep = np.ones(len(ci), dtype=bool)
    keep[d[3]] = False                                                # a row without a diagonal entry
    rp2 = np.concatenate([[0], np.cumsum(np.add.reduceat(keep.astype(np.int64), rp[:-1]))])
    assert run(rp2, ci[keep], va[keep])[3] == 1
    rp, ci, va = HC.arrow()                                           # the long row: the wave's path
    vb = va.copy()
    vb[0] = 0.0
    assert run(rp, ci, vb)[3] == 1 and run(rp, ci, va)[3] == 0


def test_entry_limit_and_argument_errors(dev):
    lib, st = dev.lib, _st(dev)
    rp, ci, va, shift, theta = _mats["lap_33x35"]
    rc, lv, _ = SA.c_plan(dev.lib, rp, ci, va)
    v = lv[0]
    n, nc = v["n"], v["nc"]
    M = _up(dev, rp, ci, va)
    ddinv, dagg = dev.arr(v["dinv"]), dev.arr(v["agg"].astype(np.int32))
    p = [C.c_void_p() for _ in range(3)]
    pnnz = C.c_int64(-1)

    def prolong(n_=n, nc_=nc, rp_=dev.ptr(M[0]), agg_=dev.ptr(dagg), limit=-1):
        return lib.hipk_amg_build_prolongation(st, n_, nc_, rp_, dev.ptr(M[1]), dev.ptr(M[2]), dev.ptr(ddinv), agg_, 0.3, limit,
                                               *(C.byref(x) for x in p), C.byref(pnnz))

    # one entry short: the stage answers 1 and keeps nothing
    assert prolong(limit=v["pnnz"] - 1) == 1 and not any(x.value for x in p) and pnnz.value == 0
    assert prolong(limit=0) == 1 and not any(x.value for x in p)
    assert prolong(limit=v["pnnz"]) == 0 and pnnz.value == v["pnnz"]
    r, c = [C.c_void_p() for _ in range(3)], [C.c_void_p() for _ in range(3)]
    cnnz = C.c_int64(-1)
    assert lib.hipk_amg_csr_transpose(st, n, nc, pnnz.value, *p, v["pnnz"] - 1, *(C.byref(x) for x in r)) == 1 and not any(x.value for x in r)
    assert lib.hipk_amg_csr_transpose(st, n, nc, pnnz.value, *p, 2 ** 40, *(C.byref(x) for x in r)) == 0      # beyond int32: INT32_MAX
    # the coarse matrix itself is one entry too large
    assert lib.hipk_amg_galerkin(st, n, nc, *(dev.ptr(a) for a in M), *p, *r, lv[1]["nnz"] - 1, *(C.byref(x) for x in c), C.byref(cnnz)) == 1
    assert not any(x.value for x in c) and cnnz.value == 0
    assert prolong(n_=0) == -1 and prolong(nc_=0) == -1 and prolong(nc_=n + 1) == -1 and prolong(rp_=None) == -1 and prolong(agg_=None) == -1
    assert prolong(n_=2 ** 31) == -1
    assert lib.hipk_amg_csr_transpose(st, 0, nc, 1, *p, -1, *(C.byref(x) for x in c)) == -1
    assert lib.hipk_amg_csr_transpose(st, n, nc, 2 ** 31, *p, -1, *(C.byref(x) for x in c)) == -1
    assert lib.hipk_amg_galerkin(st, n, nc, None, dev.ptr(M[1]), dev.ptr(M[2]), *p, *r, -1, *(C.byref(x) for x in c), C.byref(cnnz)) == -1
    rho, flag = C.c_double(0), C.c_int(0)
    assert lib.hipk_amg_level_finish(st, n, dev.ptr(M[0]), dev.ptr(M[1]), dev.ptr(M[2]), None, None, C.byref(rho), C.byref(flag)) == -1
    for x in p + r:
        lib.hipk_amg_setup_free(x)
