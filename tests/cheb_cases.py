"""The Chebyshev polynomial preconditioner restated in numpy, for the CPU and GPU test modules (test_cheb_host.py,
test_cheb_gpu.py) and the fixture generator tests/golden/make_cheb_golden.py.

Definition (include/primme_amd.h): y = p(A) x is the d-th iterate of Chebyshev iteration for (A - sigma I) y = x
started from y = 0 with the interval [lo, hi]:
    tb = (hi + lo)/2 - sigma, dl = (hi - lo)/2, s1 = tb/dl, rho_1 = 1/s1, y_0 = 0, y_1 = x/tb,
    rho_{k+1} = 1/(2 s1 - rho_k),  y_{k+1} = y_k + rho_{k+1} rho_k (y_k - y_{k-1}) + (2 rho_{k+1}/dl)(x - (A - sigma I) y_k)
for k = 1 .. d-1 (d - 1 operator applications).  Its residual polynomial is q(t) = T_d(l(t)) / T_d(l(sigma)) with l the map of
[lo, hi] onto [-1, 1] (y_1 = x/tb already has the degree-1 residual 1 - (t - sigma)/tb = T_1(l(t))/T_1(l(sigma))), so
p(t) = (1 - q(t)) / (t - sigma), a polynomial of degree d - 1."""
import ctypes as C
import os

import numpy as np

from primme_amd import _ffi as F
from primme_amd import problems
from checkers import Operator, ReferenceBackend

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "reference_cheb.json")


# ---- the definition -----------------------------------------------------------------------------------------------
def cheb_recurrence(apply, x, steps, lo, hi, sigma):
    """The recurrence in float64 / complex128.  x: (n,) or (n, nb); sigma: scalar or one per column."""
    x = np.asarray(x, dtype=np.complex128 if np.iscomplexobj(x) else np.float64)
    sigma = np.asarray(sigma, dtype=np.float64)
    tb = 0.5 * (hi + lo) - sigma
    dl = 0.5 * (hi - lo)
    s1 = tb / dl
    rho = 1.0 / s1
    yprev = np.zeros_like(x)
    y = x / tb
    for _ in range(1, steps):
        rn = 1.0 / (2.0 * s1 - rho)
        ynew = y + rn * rho * (y - yprev) + (2.0 * rn / dl) * (x - (apply(y) - sigma * y))
        yprev, y, rho = y, ynew, rn
    return y


def cheb_step_coefficients(steps, lo, hi, sigma):
    """Per step k = 1 .. steps-1 the four coefficients (cy, cp, cx, cw) of the form the kernels take,
    y_{k+1} = cy y_k + cp y_{k-1} + cx x + cw A y_k, for y_k and y_{k-1} STORED (no folding of y_1 = x/tb);
    sigma: array, one per column.  Returns (tb, list of 4-tuples of arrays)."""
    sigma = np.atleast_1d(np.asarray(sigma, dtype=np.float64))
    tb = 0.5 * (hi + lo) - sigma
    dl = 0.5 * (hi - lo)
    s1 = tb / dl
    rho = 1.0 / s1
    out = []
    for _ in range(1, steps):
        rn = 1.0 / (2.0 * s1 - rho)
        a, b = rn * rho, 2.0 * rn / dl
        out.append((1.0 + a + b * sigma, -a, b + 0 * sigma, -b + 0 * sigma))
        rho = rn
    return tb, out


def _cheb_T(d, t):
    """T_d(t) by the three-term recurrence (any real t)."""
    t = np.asarray(t, dtype=np.float64)
    a, b = np.ones_like(t), t.copy()
    if d == 0:
        return a
    for _ in range(1, d):
        a, b = b, 2.0 * t * b - a
    return b


def cheb_poly(lam, steps, lo, hi, sigma):
    """p(lam) = (1 - T_d(l(lam)) / T_d(l(sigma))) / (lam - sigma)."""
    ell = lambda t: (2.0 * np.asarray(t, dtype=np.float64) - hi - lo) / (hi - lo)      # noqa: E731
    q = _cheb_T(steps, ell(lam)) / _cheb_T(steps, ell(sigma))
    return (1.0 - q) / (np.asarray(lam) - sigma)


def cheb_spectral(lam, U, x, steps, lo, hi, sigma):
    """U p(Lambda) U^H x for one shift."""
    return U @ (cheb_poly(lam, steps, lo, hi, sigma) * (U.conj().T @ x))


def dense_of(rp, ci, va, n):
    A = np.zeros((n, n), dtype=np.asarray(va).dtype)
    rows = np.repeat(np.arange(n), np.diff(rp))
    A[rows, ci] = va
    return A


def rel_inf(a, b):
    return float(np.max(np.abs(a - b)) / np.max(np.abs(b)))


# ---- the preconditioner as an applyPreconditioner callback on HOST pointers ------------------------------------------
def clamp_shift(s, lo, hi, target):
    return min(s, lo) if target == "smallest" else max(s, hi)


def make_callback(op, dtype, steps, lo, hi, shift=None, target="smallest", counter=None):
    """BLOCK_OP that applies the numpy recurrence; shift None: the solver's ShiftsForPreconditioner, clamped as the
    library clamps them.  counter: a one-element list that counts the vectors preconditioned."""
    dtype = np.dtype(dtype)
    cplx = dtype.kind == "c"
    ctype = C.c_double if dtype in (np.float64, np.complex128) else C.c_float
    n = op.nrows

    def view(ptr, nb, ld):
        a = np.ctypeslib.as_array(C.cast(ptr, C.POINTER(ctype)), shape=(nb, ld * (2 if cplx else 1)))
        return a.view(dtype) if cplx else a

    def pc(x, ldx, y, ldy, bs, pp, ierr):
        nb = bs[0]
        if nb <= 0 or not x or not y:
            ierr[0] = 0
            return
        X, Y = view(x, nb, ldx[0]), view(y, nb, ldy[0])
        sh = pp[0].ShiftsForPreconditioner
        sig = np.array([shift if shift is not None else clamp_shift(sh[c], lo, hi, target) for c in range(nb)])
        Xc = X[:, :n].T.astype(np.complex128 if cplx else np.float64)
        Y[:, :n] = cheb_recurrence(op.apply_numpy, Xc, steps, lo, hi, sig).T
        if counter is not None:
            counter[0] += nb
        ierr[0] = 0
    return F.BLOCK_OP(pc)


class ChebReferenceBackend(ReferenceBackend):
    """The live reference with the numpy preconditioner installed as its applyPreconditioner."""

    def __init__(self, spec, target, counter=None):
        super().__init__()
        self.spec, self.target, self.counter = spec, target, counter

    def setup_operator(self, sess, p, keep, precond, view, ncols, nLocal, cons, nOC, v0, initSize):
        r = super().setup_operator(sess, p, keep, None, view, ncols, nLocal, cons, nOC, v0, initSize)
        cb = make_callback(sess.op, sess.dtype, self.spec["steps"], self.spec["lo"], self.spec["hi"], self.spec.get("shift"),
                           self.target, self.counter)
        keep.append(cb)
        p.applyPreconditioner = C.cast(cb, C.c_void_p)
        p.correctionParams.precondition = 1
        return r


# ---- the fixture cases ---------------------------------------------------------------------------------------------
# cheb: steps, lo, hi (the 5-point Laplacian's Gershgorin bound is 8) and, for the fixed mode, shift.
# LUNDA.mtx: spectrum [80.04, 2.24e8]; its three smallest eigenvalues lie below 2000 and the fourth at 6354 (numpy); hi = None:
# the Gershgorin bound 2.85e8, which the library computes itself.
# hermitian_banded_csr(96): one period of its diagonal (d_j = 2 + (j mod 97)/97) — from n = 98 on the smallest eigenvalues come in
# numerically double pairs, whose convergence histories depend on rounding and carry no parity information; spectrum
# [1.270, 5.0], lo is put into the gap between the third and the fourth eigenvalue (1.407, 1.417).
CASES = {
    "gdk_20x21_s4": dict(dims=(20, 21), kw=dict(numEvals=3, method="GD_plusK", eps=1e-8, aNorm=8.0), cheb=dict(steps=4, lo=0.2, hi=8.0)),
    "gdk_20x21_s8": dict(dims=(20, 21), kw=dict(numEvals=3, method="GD_plusK", eps=1e-8, aNorm=8.0), cheb=dict(steps=8, lo=0.2, hi=8.0)),
    "gdk_60x61_s4": dict(dims=(60, 61), kw=dict(numEvals=3, method="GD_plusK", eps=1e-8, aNorm=8.0), cheb=dict(steps=4, lo=0.1, hi=8.0)),
    "gdk_60x61_s8": dict(dims=(60, 61), kw=dict(numEvals=3, method="GD_plusK", eps=1e-8, aNorm=8.0), cheb=dict(steps=8, lo=0.1, hi=8.0)),
    "gdk_largest2": dict(dims=(20, 21), kw=dict(numEvals=2, target="largest", method="GD_plusK", eps=1e-8, aNorm=8.0),
                         cheb=dict(steps=4, lo=0.0, hi=7.8)),
    "olsen_b4": dict(dims=(20, 21), kw=dict(numEvals=4, method="GD_Olsen_plusK", maxBlockSize=4, eps=1e-8, aNorm=8.0),
                     cheb=dict(steps=4, lo=0.2, hi=8.0)),
    "jdqmr_lunda_fixed": dict(matrix="lunda", kw=dict(numEvals=3, method="JDQMR", eps=1e-10, maxMatvecs=200000),
                              cheb=dict(steps=8, lo=4000.0, hi=None, shift=0.0)),
    "zgdk_banded": dict(matrix="hermitian_banded", n=96, dtype="complex128", kw=dict(numEvals=3, method="GD_plusK", eps=1e-8),
                        cheb=dict(steps=4, lo=None, hi=None)),
    "float_20x21_s4": dict(dims=(20, 21), dtype="float32", kw=dict(numEvals=3, method="GD_plusK", eps=1e-4, aNorm=8.0),
                           cheb=dict(steps=4, lo=0.2, hi=8.0)),
}


def gershgorin_numpy(rp, ci, va, n):
    rows = np.repeat(np.arange(n), np.diff(rp))
    d = np.zeros(n)
    m = ci == rows
    d[rows[m]] = np.real(np.asarray(va)[m])
    off = np.bincount(rows[~m], weights=np.abs(np.asarray(va)[~m]), minlength=n)
    return float(np.min(d - off)), float(np.max(d + off))


def case_setup(name):
    """-> (Operator, solve kwargs, cheb spec with numbers for lo / hi, dtype, |A| for the tolerances)."""
    g = CASES[name]
    dtype = np.dtype(g.get("dtype", "float64"))
    spec = dict(g["cheb"])
    kw = dict(g["kw"])
    if "dims" in g:
        rp, ci, va, n = problems.laplacian_csr(tuple(g["dims"]))
        kw["v0"] = problems.start_vector(n)
        anorm = 8.0
    elif g["matrix"] == "lunda":
        import reference_driver_cases as RD
        rp, ci, va, n = RD.lunda()
        kw["v0"] = problems.start_vector(n)
        anorm = float(np.max(np.abs(np.linalg.eigvalsh(dense_of(rp, ci, va, n)))))
    else:
        n = g["n"]
        rp, ci, va = problems.hermitian_banded_csr(n)[:3]
        kw["v0"] = problems.complex_start_vector(n)
        lam = np.linalg.eigvalsh(dense_of(rp, ci, va, n))
        anorm = float(np.max(np.abs(lam)))
        spec["lo"] = float(np.round(0.5 * (lam[2] + lam[3]), 3))       # in the gap above the three wanted ones
    if spec["hi"] is None:
        spec["hi"] = gershgorin_numpy(rp, ci, va, n)[1]
    return Operator(n, csr=(rp, ci, va)), kw, spec, dtype, anorm


def precond_tuple(spec):
    t = ("chebyshev", spec["steps"], spec["lo"], spec["hi"])
    return t + (spec["shift"],) if spec.get("shift") is not None else t


def run_case(name, backend, counter=None):
    """backend: "reference" | "hostcheck" (numpy callback as the preconditioner) | "hip" (the library's own)."""
    from checkers import eigsh
    op, kw, spec, dtype, anorm = case_setup(name)
    target = kw.get("target", "smallest")
    if backend == "reference":
        return eigsh(op, backend=ChebReferenceBackend(spec, target, counter), dtype=dtype, **kw)
    if backend == "hostcheck":
        cb = make_callback(op, dtype, spec["steps"], spec["lo"], spec["hi"], spec.get("shift"), target, counter)
        return eigsh(op, backend="hostcheck", dtype=dtype, user_precond=cb, **kw)
    return eigsh(op, backend=backend, dtype=dtype, precond=precond_tuple(spec), **kw)
