"""The Chebyshev polynomial preconditioner of the singular value solver restated in numpy, for test_svds_cheb_host.py,
test_svds_cheb_gpu.py and the fixture generator tests/golden/make_svds_cheb_golden.py.

Definition (include/primme_amd_svds.h), in singular value units: with lo = slo^2, hi = shi^2, sigma = sshift^2
and p the polynomial of cheb_cases.cheb_recurrence (the steps-th Chebyshev iterate for (M - sigma I) y = x from y = 0)
    mode 1 (primme_svds_op_AtA)        y = p(A'A) x
    mode 2 (primme_svds_op_AAt)        y = p(AA') x
    mode 3 (primme_svds_op_augmented)  y = (B + sshift I) diag(p(A'A), p(AA')) x,  B = [0 A'; A 0], x = [v; u] (n, then m)."""
import ctypes as C
import os

import numpy as np

import cheb_cases as CC
import reference_driver_cases as RD
from checkers import ReferenceBackend, svds, transpose_csr
from primme_amd import _ffi as F
from primme_amd.problems import csr_matvec_numpy

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "reference_svds_cheb.json")
MODE_ATA, MODE_AAT, MODE_AUG = 1, 2, 3


# ---- the definition -----------------------------------------------------------------------------------------------
def svds_cheb_apply(av, atv, n, x, mode, steps, slo, shi, sshift):
    """av(v) = A v, atv(u) = A^H u on (rows, nb) blocks; x: (len, nb)."""
    lo, hi, sigma = slo * slo, shi * shi, sshift * sshift
    if mode == MODE_ATA:
        return CC.cheb_recurrence(lambda v: atv(av(v)), x, steps, lo, hi, sigma)
    if mode == MODE_AAT:
        return CC.cheb_recurrence(lambda u: av(atv(u)), x, steps, lo, hi, sigma)
    if mode != MODE_AUG:
        raise ValueError(mode)
    tv = CC.cheb_recurrence(lambda v: atv(av(v)), x[:n], steps, lo, hi, sigma)
    tu = CC.cheb_recurrence(lambda u: av(atv(u)), x[n:], steps, lo, hi, sigma)
    return np.concatenate([atv(tu) + sshift * tv, av(tv) + sshift * tu], axis=0)


def svds_cheb_spectral(A, x, mode, steps, slo, shi, sshift):
    """The same through the eigen-decomposition of A'A, AA' or B (dense A); p is evaluated by the scalar recurrence on the
    eigenvalues, which has no division by (lambda - sigma): a shift on an eigenvalue is fine."""
    m, n = A.shape
    lo, hi, sigma = slo * slo, shi * shi, sshift * sshift

    def p(lam):
        return CC.cheb_recurrence(lambda y: lam * y, np.ones_like(lam), steps, lo, hi, sigma)
    if mode == MODE_ATA or mode == MODE_AAT:
        lam, W = np.linalg.eigh(A.conj().T @ A if mode == MODE_ATA else A @ A.conj().T)
        return W @ (p(lam)[:, None] * (W.conj().T @ x.reshape(len(lam), -1))).reshape(x.shape)
    B = np.block([[np.zeros((n, n), dtype=A.dtype), A.conj().T], [A, np.zeros((m, m), dtype=A.dtype)]])
    lb, W = np.linalg.eigh(B)
    return W @ (((lb + sshift) * p(lb * lb))[:, None] * (W.conj().T @ x.reshape(m + n, -1))).reshape(x.shape)


def csr_applies(m, n, rp, ci, va):
    """(av, atv) of a CSR matrix in float64 / complex128; atv applies the conjugate transpose"""
    wide = np.complex128 if np.iscomplexobj(va) else np.float64
    va = np.asarray(va).astype(wide)
    rpT, ciT, vaT = transpose_csr(m, n, rp, ci, va)
    vaT = np.conj(vaT)
    return (lambda v: csr_matvec_numpy(rp, ci, va, v.reshape(n, -1).astype(wide)).reshape(m, *v.shape[1:]),
            lambda u: csr_matvec_numpy(rpT, ciT, vaT, u.reshape(m, -1).astype(wide)).reshape(n, *u.shape[1:]))


def norm_bound_numpy(m, n, rp, ci, va):
    """sqrt(|A|_1 |A|_inf) as the library forms it: absolute row sums of A and of A'; a complex entry a + ib counts |a| + |b|
    (the library sees the real-equivalent form)"""
    a = np.abs(np.real(va)).astype(np.float64) + (np.abs(np.imag(va)).astype(np.float64) if np.iscomplexobj(va) else 0.0)
    rows = np.repeat(np.arange(m), np.diff(rp))
    rinf = float(np.max(np.bincount(rows, weights=a, minlength=m))) if m else 0.0
    r1 = float(np.max(np.bincount(ci, weights=a, minlength=n))) if n else 0.0
    return float(np.sqrt(rinf * r1))


# ---- the preconditioner as an applyPreconditioner callback on HOST pointers ------------------------------------------
def make_callback(m, n, csr, dtype, steps, slo, shi, sshift, counter=None):
    """SVDS_BLOCK_OP that applies the restatement; counter: a one-element list that counts the vectors preconditioned."""
    dtype = np.dtype(dtype)
    cplx = dtype.kind == "c"
    ctype = C.c_double if dtype in (np.float64, np.complex128) else C.c_float
    av, atv = csr_applies(m, n, *csr)
    length = {MODE_ATA: n, MODE_AAT: m, MODE_AUG: m + n}

    def view(ptr, nb, ld):
        a = np.ctypeslib.as_array(C.cast(ptr, C.POINTER(ctype)), shape=(nb, ld * (2 if cplx else 1)))
        return a.view(dtype) if cplx else a

    def pc(x, ldx, y, ldy, bs, mode, pp, ierr):
        nb = bs[0]
        if nb <= 0 or not x or not y:
            ierr[0] = 0
            return
        if mode[0] not in length:
            ierr[0] = 1
            return
        ln = length[mode[0]]
        X, Y = view(x, nb, ldx[0]), view(y, nb, ldy[0])
        Xc = X[:, :ln].T.astype(np.complex128 if cplx else np.float64)
        Y[:, :ln] = svds_cheb_apply(av, atv, n, Xc, mode[0], steps, slo, shi, sshift).T
        if counter is not None:
            counter[0] += nb
        ierr[0] = 0
    return F.SVDS_BLOCK_OP(pc)


class SvdsChebReferenceBackend(ReferenceBackend):
    """The live reference with the numpy preconditioner installed as its applyPreconditioner."""

    def __init__(self, spec, counter=None):
        super().__init__()
        self.spec, self.counter = spec, counter

    def setup_svds_operator(self, ps, keep, m, n, rp, ci, va, ctype, precond, dtype):
        solver = super().setup_svds_operator(ps, keep, m, n, rp, ci, va, ctype, None, dtype)
        cb = make_callback(m, n, (rp, ci, va), dtype, self.spec["steps"], self.spec["slo"], self.spec["shi"], self.spec["sshift"],
                           self.counter)
        keep.append(cb)
        ps.applyPreconditioner = C.cast(cb, C.c_void_p)
        return solver


# ---- matrices -------------------------------------------------------------------------------------------------------
def difference_matrix(n):
    """D, (n+1) x n, D[i,i] = 1, D[i+1,i] = -1: D'D is the 1-D Laplacian, sigma_k = 2 sin(k pi / (2 (n+1))); every row and column sum
    of squares is <= 2 (Jacobi is the identity up to scale); |D|_1 = |D|_inf = 2, so the norm bound is exactly 2."""
    rp = np.concatenate([[0, 1], 1 + 2 * np.arange(1, n), [2 * n]]).astype(np.int32)
    ci = np.concatenate([[0], np.stack([np.arange(n - 1), np.arange(1, n)], axis=1).reshape(-1), [n - 1]]).astype(np.int32)
    va = np.concatenate([[1.0], np.tile([-1.0, 1.0], n - 1), [-1.0]])
    return n + 1, n, (rp, ci, va)


def dense_of(m, n, csr):
    rp, ci, va = csr
    A = np.zeros((m, n), dtype=np.asarray(va).dtype)
    A[np.repeat(np.arange(m), np.diff(rp)), ci] = va
    return A


def _matrix(g):
    import test_svds_host as TS
    kind = g["matrix"]
    if kind == "D":
        return difference_matrix(g["n"])
    if kind == "rect":
        A, csr = TS._rect(*g["shape"])
        return g["shape"][0], g["shape"][1], csr
    if kind == "rect_complex":
        Z, csr = TS._rect_complex(*g["shape"])
        return g["shape"][0], g["shape"][1], csr
    rp, ci, va, m, n = RD.svds_matrix("rect.mtx")
    return m, n, (rp, ci, va)


# ---- the fixture cases ---------------------------------------------------------------------------------------------
# D, 3 smallest: slo = 0.055 lies between sigma_3 = 0.04689 and sigma_4 = 0.06251, shi = None (the norm bound, 2), sshift = 0.
# The largest-target cases: slo = 0, shi = the midpoint of the last wanted singular value and the next one (numpy.linalg.svd),
# sshift = the norm bound.
_GD = dict(methodStage1="GD_plusK")
CASES = {
    "D200_s4": dict(matrix="D", n=200, kw=dict(numSvals=3, target="smallest", eps=1e-8, **_GD), cheb=dict(steps=4, slo=0.055, shi=None)),
    "D200_s8": dict(matrix="D", n=200, kw=dict(numSvals=3, target="smallest", eps=1e-8, **_GD), cheb=dict(steps=8, slo=0.055, shi=None)),
    "rect300x200": dict(matrix="rect", shape=(300, 200), kw=dict(numSvals=4, target="largest", eps=1e-10, **_GD), cheb=dict(steps=4, slo=0.0)),
    "rect300x200_hybrid": dict(matrix="rect", shape=(300, 200), kw=dict(numSvals=4, target="largest", eps=1e-10, method="hybrid", **_GD),
                               cheb=dict(steps=4, slo=0.0)),
    "rect300x200_augmented": dict(matrix="rect", shape=(300, 200), kw=dict(numSvals=4, target="largest", eps=1e-9, method="augmented", **_GD),
                                  cheb=dict(steps=4, slo=0.0)),
    "rect200x300": dict(matrix="rect", shape=(200, 300), kw=dict(numSvals=4, target="largest", eps=1e-10, **_GD), cheb=dict(steps=4, slo=0.0)),
    "rect_mtx": dict(matrix="rect.mtx", kw=dict(numSvals=5, target="largest", eps=1e-10, **_GD), cheb=dict(steps=4, slo=0.0)),
    "float_rect300x200": dict(matrix="rect", shape=(300, 200), dtype="float32", kw=dict(numSvals=4, target="largest", eps=1e-4, **_GD),
                              cheb=dict(steps=4, slo=0.0)),
    "z_rect120x80": dict(matrix="rect_complex", shape=(120, 80), dtype="complex128", kw=dict(numSvals=4, target="largest", eps=1e-10, **_GD),
                         cheb=dict(steps=4, slo=0.0)),
}

_setup_cache = {}


def case_setup(name):
    """-> (m, n, csr, solve kwargs, spec with numbers for slo / shi / sshift, dtype, |A|_2, the tuple for precond=)."""
    if name in _setup_cache:
        return _setup_cache[name]
    g = CASES[name]
    dtype = np.dtype(g.get("dtype", "float64"))
    m, n, (rp, ci, va) = _matrix(g)
    va = np.asarray(va).astype(dtype)                     # what the library is handed
    s = np.linalg.svd(dense_of(m, n, (rp, ci, va)).astype(np.complex128 if dtype.kind == "c" else np.float64), compute_uv=False)
    kw = dict(g["kw"])
    spec = dict(g["cheb"])
    bound = norm_bound_numpy(m, n, rp, ci, va)
    k = kw["numSvals"]
    if kw["target"] == "largest":
        spec["shi"] = float(0.5 * (s[k - 1] + s[k]))
        spec["sshift"] = bound
        tup = ("chebyshev", spec["steps"], spec["slo"], spec["shi"])             # sshift omitted: the norm bound
    else:
        assert spec["shi"] is None
        spec["shi"] = bound
        spec["sshift"] = 0.0
        tup = ("chebyshev", spec["steps"], spec["slo"], None)                    # shi None: the norm bound; sshift omitted: 0
    _setup_cache[name] = (m, n, (rp, ci, va), kw, spec, dtype, float(s[0]), tup)
    return _setup_cache[name]


def run_case(name, backend, counter=None, plain=False):
    """backend: "reference" | "hostcheck" (numpy callback as the preconditioner) | "hip" (the library's own); plain: no
    preconditioner at all."""
    m, n, csr, kw, spec, dtype, _, tup = case_setup(name)
    if plain:
        return svds(m, n, csr, backend=backend, dtype=dtype, **kw)
    if backend == "reference":
        return svds(m, n, csr, backend=SvdsChebReferenceBackend(spec, counter), dtype=dtype, **kw)
    if backend == "hostcheck":
        cb = make_callback(m, n, csr, dtype, spec["steps"], spec["slo"], spec["shi"], spec["sshift"], counter)
        return svds(m, n, csr, backend="hostcheck", dtype=dtype, user_precond=cb, **kw)
    return svds(m, n, csr, backend=backend, dtype=dtype, precond=tup, **kw)
