"""Helpers for the aggregation algebraic multigrid preconditioner (csrc/csr_tools.c:
primme_amd_amg_plan_create, csrc/hipk_amg.hip, primme_amd_amg_precond in csrc/amd_operator.hip): the plan read from the library
into numpy arrays, the test matrices, and a dense numpy restatement of the cycle built from the plan's maps: the level
matrices M_l, the 0/1 prolongations P_l, the Chebyshev polynomials for D^-1 M_l on [rho_l / 4, rho_l] and the V-cycle, applied
to a block of vectors or, applied to the identity, as the matrix K.  Every function of the restatement takes the dtype it
computes in (float32, float64, longdouble), so that the cycle's own rounding level can be measured."""
import ctypes as C
import os

import numpy as np

from primme_amd import problems

MAXLEVELS = 24
DENSE_ROWS = 256
LUNDA = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "reference_driver", "LUNDA.mtx")


class Level(C.Structure):
    _fields_ = [("n", C.c_int64), ("nnz", C.c_int64), ("nc", C.c_int64), ("rowptr", C.POINTER(C.c_int32)),
                ("colind", C.POINTER(C.c_int32)), ("values", C.POINTER(C.c_double)), ("dinv", C.POINTER(C.c_double)),
                ("rho", C.c_double), ("agg", C.POINTER(C.c_int32)), ("aggptr", C.POINTER(C.c_int32)),
                ("aggrows", C.POINTER(C.c_int32))]


class Plan(C.Structure):
    _fields_ = [("nlevels", C.c_int), ("shift", C.c_double), ("theta", C.c_double), ("level", Level * MAXLEVELS)]


def _copy(p, n, dt):
    return np.ctypeslib.as_array(p, shape=(max(int(n), 1),))[:int(n)].astype(dt, copy=True)


def c_plan(lib, rp, ci, va, shift=0.0, theta=0.08):
    """(rc, levels): the plan of the library as a list of dicts of numpy arrays (copies; the plan is freed); values may be
    float64 or float32"""
    lib.primme_amd_amg_plan_create.argtypes = [C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_double, C.c_double,
                                               C.POINTER(C.POINTER(Plan))]
    lib.primme_amd_amg_plan_create.restype = C.c_int
    lib.primme_amd_amg_plan_free.argtypes = [C.POINTER(Plan)]
    lib.primme_amd_amg_plan_free.restype = None
    lib.primme_amd_amg_coarse_inverse.argtypes = [C.POINTER(Plan), C.c_void_p]
    lib.primme_amd_amg_coarse_inverse.restype = C.c_int
    rp = np.ascontiguousarray(rp, dtype=np.int32)
    ci = np.ascontiguousarray(ci, dtype=np.int32)
    va = np.ascontiguousarray(va)
    assert va.dtype in (np.float64, np.float32)
    P = C.POINTER(Plan)()
    rc = lib.primme_amd_amg_plan_create(len(rp) - 1, rp.ctypes.data_as(C.c_void_p), ci.ctypes.data_as(C.c_void_p),
                                        va.ctypes.data_as(C.c_void_p), va.dtype.itemsize, shift, theta, C.byref(P))
    if rc:
        assert not P
        return rc, None
    levels = []
    for l in range(P.contents.nlevels):
        L = P.contents.level[l]
        d = dict(n=int(L.n), nnz=int(L.nnz), nc=int(L.nc), rho=float(L.rho), rowptr=_copy(L.rowptr, L.n + 1, np.int64),
                 colind=_copy(L.colind, L.nnz, np.int64), values=_copy(L.values, L.nnz, np.float64),
                 dinv=_copy(L.dinv, L.n, np.float64))
        if L.nc > 0:
            d.update(agg=_copy(L.agg, L.n, np.int64), aggptr=_copy(L.aggptr, L.nc + 1, np.int64), aggrows=_copy(L.aggrows, L.n, np.int64))
        else:
            assert not L.agg and not L.aggptr and not L.aggrows
        levels.append(d)
    nl = levels[-1]["n"]
    if nl <= DENSE_ROWS:
        G = np.full((nl, nl), np.nan)
        levels[-1]["G_rc"] = lib.primme_amd_amg_coarse_inverse(P, G.ctypes.data_as(C.c_void_p))
        levels[-1]["G"] = G
    lib.primme_amd_amg_plan_free(P)
    return 0, levels


def dense(n, rp, ci, va, dt=np.float64):
    A = np.zeros((n, n), dtype=dt)
    rows = np.repeat(np.arange(n), np.diff(rp))
    np.add.at(A, (rows, np.asarray(ci, dtype=np.int64)), np.asarray(va).astype(dt))
    return A


def lunda():
    rp, ci, va, n, _ = problems.read_matrix_market(LUNDA)
    return rp, ci, va


def lunda_tiled(ntiles=4):
    """the block-diagonal tiling of LUNDA.mtx, tile t scaled by 1 + t / 4"""
    rp, ci, va = lunda()
    return problems.tile_block_diagonal(rp, ci, va, ntiles, scale_fn=lambda t: 1.0 + 0.25 * t)


def matrices():
    """name -> (rowptr, colind, values) of the plan tests"""
    i = np.arange(12 * 13)
    V = 0.5 + 0.4 * np.sin(0.37 * (i % 12)) * np.cos(0.23 * (i // 12))
    out = {}
    for name, dims in (("lap1d_1", (1,)), ("lap1d_2", (2,)), ("lap1d_5", (5,)), ("lap_6x7", (6, 7)), ("lap_33x35", (33, 35)),
                       ("lap_5x4x3", (5, 4, 3))):
        out[name] = problems.laplacian_csr(dims)[:3]
    out["schrodinger_12x13"] = problems.schrodinger_csr((12, 13), V)[:3]
    out["lunda"] = lunda()
    out["lunda_x4"] = lunda_tiled(4)
    out["diag_300"] = (np.arange(301), np.arange(300), 1.0 + np.arange(300) / 7.0)
    return out


def prolongation(agg, nc, dt=np.float64):
    P = np.zeros((len(agg), nc), dtype=dt)
    P[np.arange(len(agg)), agg] = 1
    return P


def chol_inverse(M):
    """inverse of a symmetric positive definite matrix from its Cholesky factor, in M's dtype (longdouble included)"""
    n = M.shape[0]
    L = np.zeros_like(M)
    for j in range(n):
        d = M[j, j] - L[j, :j] @ L[j, :j]
        assert d > 0
        L[j, j] = np.sqrt(d)
        L[j + 1:, j] = (M[j + 1:, j] - L[j + 1:, :j] @ L[j, :j]) / L[j, j]
    Li = np.zeros_like(M)
    for i in range(n):
        e = np.zeros(n, dtype=M.dtype)
        e[i] = 1
        Li[i] = (e - L[i, :i] @ Li[:i]) / L[i, i]
    G = Li.T @ Li
    return (G + G.T) / 2


def cheb(M, dinv, b, steps, rho, y0=None):
    """the steps-th iterate of the Chebyshev iteration for D^-1 M y = D^-1 b on [rho / 4, rho], from zero or from y0, in b's dtype"""
    dt = b.dtype.type
    hi, lo = dt(rho), dt(0.25) * dt(rho)
    tb, dl = dt(0.5) * (hi + lo), dt(0.5) * (hi - lo)
    d = dinv[:, None]
    if y0 is None:
        yp, y = np.zeros_like(b), d * b / tb
    else:
        yp, y = y0, y0 + d * (b - M @ y0) / tb
    r = dl / tb
    for _ in range(1, steps):
        rn = dt(1) / (dt(2) * tb / dl - r)
        yn = y + (rn * r) * (y - yp) + (dt(2) * rn / dl) * (d * (b - M @ y))
        yp, y, r = y, yn, rn
    return y


class Hierarchy:
    """the cycle of primme_amd_amg_precond on the levels of a plan (c_plan), in the dtype dt"""

    def __init__(self, levels, smooth_steps=2, coarse_steps=16, over=1.0, dt=np.float64):
        self.nu, self.cs, self.over, self.dt = smooth_steps, coarse_steps, dt(over), dt
        self.L = len(levels) - 1
        self.M = [dense(v["n"], v["rowptr"], v["colind"], v["values"], dt) for v in levels]
        self.dinv = [v["dinv"].astype(dt) for v in levels]
        self.rho = [v["rho"] for v in levels]
        self.P = [prolongation(v["agg"], v["nc"], dt) for v in levels[:-1]]
        self.G = None
        if levels[-1]["n"] <= DENSE_ROWS:
            # the device keeps G in double whatever the panel type is: computed in at least double, rounded to dt
            wide = np.longdouble if dt == np.longdouble else np.float64
            self.G = chol_inverse(dense(levels[-1]["n"], levels[-1]["rowptr"], levels[-1]["colind"], levels[-1]["values"], wide)).astype(dt)

    def vcycle(self, b, l=0):
        M, dinv, rho = self.M[l], self.dinv[l], self.rho[l]
        if l == self.L:
            return self.G @ b if self.G is not None else cheb(M, dinv, b, self.cs, rho)
        y = cheb(M, dinv, b, self.nu, rho)
        y = y + self.over * (self.P[l] @ self.vcycle(self.P[l].T @ (b - M @ y), l + 1))
        return cheb(M, dinv, b, self.nu, rho, y0=y)

    def matrix(self):
        return self.vcycle(np.eye(self.M[0].shape[0], dtype=self.dt))
