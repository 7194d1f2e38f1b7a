"""A dense numpy restatement of the geometric multigrid preconditioner (csrc/csr_tools.c:
primme_amd_mg_plan, csrc/hipk_mg.hip, primme_amd_multigrid_precond in csrc/amd_operator.hip), built from Kronecker products of
1-D operators: the level plan, the transfers P and R, the level operators M_l, the Chebyshev polynomials and the V-cycle,
applied to a block of vectors or, applied to the identity, as the matrix K.  Every function takes the dtype it computes in
(float32, float64, longdouble), so that the V-cycle's own rounding level can be measured.  x is the fastest index."""
import ctypes as C

import numpy as np

MAXLEVELS = 24
COARSE_POINTS = 32


def plan(dims):
    """levels [(n, w)]: n the three grid lengths, w the three weights of the 1-D Laplacians"""
    n = [tuple(int(d) for d in dims)]
    w = [(1.0, 1.0, 1.0)]
    while len(n) < MAXLEVELS and any(d >= 3 for d in n[-1]) and int(np.prod(n[-1])) > COARSE_POINTS:
        fine = n[-1]
        w.append(tuple(wd / 4 if d >= 3 else wd for d, wd in zip(fine, w[-1])))
        n.append(tuple(d // 2 if d >= 3 else d for d in fine))
    return n, w


def c_plan(lib, dims):
    """the same from the library: primme_amd_mg_plan"""
    lib.primme_amd_mg_plan.argtypes = [C.POINTER(C.c_int), C.POINTER(C.c_int), C.c_void_p, C.c_void_p]
    lib.primme_amd_mg_plan.restype = C.c_int
    n = np.full((MAXLEVELS, 3), -7, dtype=np.int32)
    w = np.full((MAXLEVELS, 3), np.nan)
    nl = C.c_int(-1)
    rc = lib.primme_amd_mg_plan((C.c_int * 3)(*dims), C.byref(nl), n.ctypes.data_as(C.c_void_p), w.ctypes.data_as(C.c_void_p))
    if rc:
        return rc, None, None
    # nothing behind the last level is touched
    assert np.all(n[nl.value:] == -7) and np.all(np.isnan(w[nl.value:]))
    return 0, [tuple(int(v) for v in r) for r in n[:nl.value]], [tuple(float(v) for v in r) for r in w[:nl.value]]


def lap1(n, dt=np.float64):
    return (2 * np.eye(n) - np.eye(n, k=1) - np.eye(n, k=-1)).astype(dt)


def prolong1(n, dt=np.float64):
    """n x (n // 2) linear interpolation: coarse j sits on fine 2 j + 1"""
    nc = n // 2
    P = np.zeros((n, nc), dtype=dt)
    for i in range(n):
        if i % 2:
            P[i, (i - 1) // 2] = 1
        else:
            if i // 2 - 1 >= 0: P[i, i // 2 - 1] = 0.5
            if i // 2 < nc: P[i, i // 2] = 0.5
    return P


def kron3(ax, ay, az):
    return np.kron(az, np.kron(ay, ax))


def eye3(n, dt):
    return [np.eye(d, dtype=dt) for d in n]


def weighted_laplacian(n, w, dt=np.float64):
    """sum_d w_d L_d over the dimensions with n_d > 1"""
    m = int(np.prod(n))
    A = np.zeros((m, m), dtype=dt)
    for d in range(3):
        if n[d] > 1:
            f = eye3(n, dt)
            f[d] = lap1(n[d], dt)
            A += dt(w[d]) * kron3(*f)
    return A


def level_operator(n, w, scale=1.0, shift=0.0, dt=np.float64):
    return dt(scale) * weighted_laplacian(n, w, dt) + dt(shift) * np.eye(int(np.prod(n)), dtype=dt)


def coarsened(nf):
    return [d >= 3 for d in nf]


def prolongation(nf, dt=np.float64):
    return kron3(*[prolong1(d, dt) if d >= 3 else np.eye(d, dtype=dt) for d in nf])


def restriction(nf, dt=np.float64):
    return kron3(*[(dt(0.5) * prolong1(d, dt).T) if d >= 3 else np.eye(d, dtype=dt) for d in nf])


def spectrum_ends(n, w, scale, shift):
    """exact smallest and largest eigenvalue of the level operator, and D = the number of dimensions with n > 1"""
    lo = hi = 0.0
    D = 0
    for d in range(3):
        if n[d] > 1:
            c = np.cos(np.pi / (n[d] + 1))
            lo += w[d] * (2 - 2 * c)
            hi += w[d] * (2 + 2 * c)
            D += 1
    return scale * lo + shift, scale * hi + shift, D


def cheb(M, b, steps, lo, hi, y0=None):
    """the steps-th iterate of the Chebyshev iteration for M y = b on [lo, hi], from zero or from y0, in b's dtype"""
    dt = b.dtype.type
    tb, dl = dt(0.5 * (hi + lo)), dt(0.5 * (hi - lo))
    if y0 is None:
        y = b / tb
        done = 1
    else:
        y = y0 + (b - M @ y0) / tb
        done = 1
    if dl <= 0 or steps == 1:
        return y
    yp = np.zeros_like(b) if y0 is None else y0
    s1 = tb / dl
    rho = dl / tb
    for _ in range(done, steps):
        rn = dt(1) / (dt(2) * s1 - rho)
        yn = y + (rn * rho) * (y - yp) + (dt(2) * rn / dl) * (b - M @ y)
        yp, y, rho = y, yn, rn
    return y


class Hierarchy:
    def __init__(self, dims, smooth_steps=2, coarse_steps=16, scale=1.0, shift=0.0, dt=np.float64):
        self.n, self.w = plan(dims)
        self.nu, self.cs, self.scale, self.shift, self.dt = smooth_steps, coarse_steps, scale, shift, dt
        self.L = len(self.n) - 1
        self.M = [level_operator(n, w, scale, shift, dt) for n, w in zip(self.n, self.w)]
        self.P = [prolongation(self.n[l], dt) for l in range(self.L)]
        self.R = [restriction(self.n[l], dt) for l in range(self.L)]
        self.ends = [spectrum_ends(n, w, scale, shift) for n, w in zip(self.n, self.w)]

    def vcycle(self, b, l=0):
        lo, hi, D = self.ends[l]
        if l == self.L:
            return cheb(self.M[l], b, self.cs, lo, hi)
        slo = hi / (2 * D)
        y = cheb(self.M[l], b, self.nu, slo, hi)
        y = y + self.P[l] @ self.vcycle(self.R[l] @ (b - self.M[l] @ y), l + 1)
        return cheb(self.M[l], b, self.nu, slo, hi, y0=y)

    def matrix(self):
        return self.vcycle(np.eye(self.M[0].shape[0], dtype=self.dt))
