"""Helpers for smoothed aggregation (csrc/csr_tools.c: primme_amd_amg_plan_create_smoothed, csrc/hipk_amg.hip:
hipk_amg_csr_apply), on top of tests/amg_cases.py: the whole plan structure with its transfer matrices read into numpy arrays,
and the dense restatement of the cycle with the plan's own P_l in place of the 0/1 matrices."""
import ctypes as C

import numpy as np

import amg_cases as AMG

OMEGA = 4.0 / 3.0


class Transfer(C.Structure):
    _fields_ = [("pnnz", C.c_int64), ("prowptr", C.POINTER(C.c_int32)), ("pcolind", C.POINTER(C.c_int32)),
                ("pvalues", C.POINTER(C.c_double)), ("rrowptr", C.POINTER(C.c_int32)), ("rcolind", C.POINTER(C.c_int32)),
                ("rvalues", C.POINTER(C.c_double))]


class Plan(C.Structure):
    """the whole of primme_amd_amg_plan; its head is amg_cases.Plan"""
    _fields_ = AMG.Plan._fields_ + [("omega", C.c_double), ("transfer", Transfer * AMG.MAXLEVELS)]


def _declare(lib):
    head = [C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_double, C.c_double]
    lib.primme_amd_amg_plan_create.argtypes = head + [C.c_void_p]
    lib.primme_amd_amg_plan_create.restype = C.c_int
    lib.primme_amd_amg_plan_create_smoothed.argtypes = head + [C.c_double, C.c_void_p]
    lib.primme_amd_amg_plan_create_smoothed.restype = C.c_int
    lib.primme_amd_amg_plan_free.argtypes = [C.c_void_p]
    lib.primme_amd_amg_plan_free.restype = None
    lib.primme_amd_amg_coarse_inverse.argtypes = [C.c_void_p, C.c_void_p]
    lib.primme_amd_amg_coarse_inverse.restype = C.c_int


def c_plan(lib, rp, ci, va, shift=0.0, theta=0.08, omega=OMEGA):
    """(rc, levels, omega of the plan): the levels as amg_cases.c_plan gives them; where the plan has transfer matrices a level
    but the last also holds P = (prowptr, pcolind, pvalues) and R = (rrowptr, rcolind, rvalues), else "transfer_null": True.
    omega = None asks for the plain plan."""
    _declare(lib)
    rp = np.ascontiguousarray(rp, dtype=np.int32)
    ci = np.ascontiguousarray(ci, dtype=np.int32)
    va = np.ascontiguousarray(va)
    assert va.dtype in (np.float64, np.float32)
    P = C.POINTER(Plan)()
    args = (len(rp) - 1, rp.ctypes.data_as(C.c_void_p), ci.ctypes.data_as(C.c_void_p), va.ctypes.data_as(C.c_void_p), va.dtype.itemsize,
            shift, theta)
    if omega is None:
        rc = lib.primme_amd_amg_plan_create(*args, C.byref(P))
    else:
        rc = lib.primme_amd_amg_plan_create_smoothed(*args, omega, C.byref(P))
    if rc:
        assert not P
        return rc, None, None
    levels = []
    cp = AMG._copy
    for l in range(AMG.MAXLEVELS):
        L, X = P.contents.level[l], P.contents.transfer[l]
        if l >= P.contents.nlevels:
            assert not L.rowptr and not X.prowptr and not X.rrowptr
            continue
        d = dict(n=int(L.n), nnz=int(L.nnz), nc=int(L.nc), rho=float(L.rho), rowptr=cp(L.rowptr, L.n + 1, np.int64),
                 colind=cp(L.colind, L.nnz, np.int64), values=cp(L.values, L.nnz, np.float64), dinv=cp(L.dinv, L.n, np.float64))
        if L.nc > 0:
            d.update(agg=cp(L.agg, L.n, np.int64), aggptr=cp(L.aggptr, L.nc + 1, np.int64), aggrows=cp(L.aggrows, L.n, np.int64))
        else:
            assert not L.agg and not L.aggptr and not L.aggrows
        if L.nc > 0 and X.prowptr:
            d.update(pnnz=int(X.pnnz), prowptr=cp(X.prowptr, L.n + 1, np.int64), pcolind=cp(X.pcolind, X.pnnz, np.int64),
                     pvalues=cp(X.pvalues, X.pnnz, np.float64), rrowptr=cp(X.rrowptr, L.nc + 1, np.int64),
                     rcolind=cp(X.rcolind, X.pnnz, np.int64), rvalues=cp(X.rvalues, X.pnnz, np.float64))
        else:
            assert not (X.prowptr or X.pcolind or X.pvalues or X.rrowptr or X.rcolind or X.rvalues) and X.pnnz == 0
            d["transfer_null"] = True
        levels.append(d)
    nl = levels[-1]["n"]
    if nl <= AMG.DENSE_ROWS:
        G = np.full((nl, nl), np.nan)
        levels[-1]["G_rc"] = lib.primme_amd_amg_coarse_inverse(P, G.ctypes.data_as(C.c_void_p))
        levels[-1]["G"] = G
    om = float(P.contents.omega)
    lib.primme_amd_amg_plan_free(P)
    return 0, levels, om


def dense_rect(nr, ncol, rp, ci, va, dt=np.float64):
    A = np.zeros((nr, ncol), dtype=dt)
    rows = np.repeat(np.arange(nr), np.diff(rp))
    np.add.at(A, (rows, np.asarray(ci, dtype=np.int64)), np.asarray(va).astype(dt))
    return A


class Hierarchy(AMG.Hierarchy):
    """the cycle on the levels of a smoothed plan: amg_cases.Hierarchy with the plan's P_l (double values, rounded to dt as the
    device rounds them when it multiplies in double: not at all for float64 and longdouble) and over = 1"""

    def __init__(self, levels, smooth_steps=2, coarse_steps=16, dt=np.float64):
        super().__init__(levels, smooth_steps, coarse_steps, 1.0, dt)
        # the device keeps P in double whatever the panel type is and multiplies in double
        wide = np.longdouble if dt == np.longdouble else np.float64
        self.Pw = [dense_rect(v["n"], v["nc"], v["prowptr"], v["pcolind"], v["pvalues"], wide) for v in levels[:-1]]

    def vcycle(self, b, l=0):
        M, dinv, rho = self.M[l], self.dinv[l], self.rho[l]
        if l == self.L:
            return self.G @ b if self.G is not None else AMG.cheb(M, dinv, b, self.cs, rho)
        dt = b.dtype
        y = AMG.cheb(M, dinv, b, self.nu, rho)
        # the transfers sum in (at least) double and round once to the panel type
        bc = (self.Pw[l].T @ (b - M @ y).astype(self.Pw[l].dtype)).astype(dt)
        yc = self.vcycle(bc, l + 1)
        y = (y.astype(self.Pw[l].dtype) + self.Pw[l] @ yc.astype(self.Pw[l].dtype)).astype(dt)
        return AMG.cheb(M, dinv, b, self.nu, rho, y0=y)
