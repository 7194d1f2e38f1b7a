"""Cases, operand layouts and high-precision references for the branch-by-branch tests of the COMPLEX panel, Ritz and
column kernels (csrc/hipk_complex.hip, HIPK_C64 / HIPK_C32) and of hipk_copy_cols (csrc/hipk_vec.hip, all four types):
tests/test_complex_branches_host.py runs them on the plain-C oracle, tests/test_complex_branches_gpu.py on the device.
The structure is that of tests/panel_branch_cases.py, whose Operand / small / gamma / Report / run_cases are used here.

Layouts.  Every operand sits inside [guard | operand | guard]; guards, the rows [m, ld), unused columns and spare output
slots are NaN in BOTH halves of a complex element, and everything a call must not write is compared bit for bit
afterwards (either half differing counts).  The complex code keys on nothing but sizes, so the flavours are: 'eq'
(ld == m), 'odd' and 'even' (ld > m), and for HIPK_C32 'shift' (base moved by one element = 8 bytes: the only alignment a
cpx<float> load can lose).  Coefficients, h, M, axpy factors and inner products are (re, im) pairs = complex128 operands
with leading dimensions in pairs and spare NaN slots behind each column; theta, scale factors and squared norms are real.

References (np.clongdouble, from include/primme_amd_kernels.h, NOT from the kernels and not from
oracle/hipk_cpu_complex.c; on the inputs already rounded to the panel type).  Panels come as (ncols, m) arrays.
Conventions they state: the LEFT operand of an inner product is conjugated (col_j^H X, x^H y); coefficients multiply
unconjugated; M[q + c nx] = M(q, c); theta, scale factors and norms are real.  Each returns with the result the sum of
absolute real terms S of every component, as a complex number: S.real belongs to the real part, S.imag to the imaginary
part (for p q: |pr||qr| + |pi||qi| and |pr||qi| + |pi||qr|).  Operands are asymmetric (independent real and imaginary
parts, a different magnitude per column, a non-Hermitian M, theta distinct per column), so that a swapped conjugate or
re/im, a transposed M or a row <-> column swap cannot cancel.

Tolerances (derived, nothing tuned), with gamma(n, u) = n u / (1 - n u), u64 = 2^-53, uT = unit round-off of the real type
of the panel.  One component of a complex sum of n terms is a real sum of 2 n products, so the formulae of
panel_branch_cases.py hold with 2 n for n:
  * element-wise output of n complex terms, rounded to T:                 2 gamma(2 n + 2, uT) S
  * reduction over m rows (double accumulation by contract) of inputs:    2 gamma(2 m + 2, u64) S
  * reduction whose operand is a computed vector of n terms per element:  2 (gamma(2 m + 2, u64) + gamma(2 n + 2, uT)) S
The factor 2 is for the reference's own error, fused against unfused products, and the second computed factor of r^H r.
n per operation: project tot (X and tot products); project_mul tot + nx (a component of X - [segs] coef is off by
gamma(2 tot + 1) S, the sum of 2 nx products with M adds gamma(2 nx), the store one rounding); XV / XW jobs k, residual
jobs 2 k (W h and theta V h); axpy, xpay, scale, residual_cols 1; scale by 1/sqrt: 2 (the factor takes two more roundings).
"""
import ctypes as C
import zlib

import numpy as np

from primme_amd import _ffi as F
import panel_branch_cases as P
from panel_branch_cases import Operand, small, gamma, Report, GUARD, U64, run_cases as _run_cases   # noqa: F401

LD, CLD = np.longdouble, np.clongdouble
C64, C32, F64, F32 = F.HIPK_C64, F.HIPK_C32, F.HIPK_F64, F.HIPK_F32
NPDT = {C64: np.complex128, C32: np.complex64, F64: np.float64, F32: np.float32}
UNIT = {C64: 2.0 ** -53, C32: 2.0 ** -24}
TNAME = {C64: "c64", C32: "c32", F64: "f64", F32: "f32"}
ZTYPES = [C64, C32]
FLAVOURS = {C64: ["eq", "odd", "even"], C32: ["eq", "odd", "even", "shift"]}
XV, XW, RES = F.HIPK_JOB_XV, F.HIPK_JOB_XW, F.HIPK_JOB_RES
ZPROJ_LDS = 2048          # HIPK_Z_PROJECT_MAXCOEF of the header
UTIL_MAXCOLS = 64         # csrc/hipk_panel_dev.h (test_case_tables... reads the header and compares)
COPY_MIN_BYTES = 4096     # hipk_copy_cols: shorter columns go to the runtime's 2-D copy


def zbound_elem(dt, n, S):
    return 2.0 * gamma(2 * n + 2, UNIT[dt]) * S


def zbound_red(m, S, dt=None, n=None):
    g = gamma(2 * m + 2, U64)
    if n is not None:
        g += gamma(2 * n + 2, UNIT[dt])
    return 2.0 * g * S


def zcmp(rep, what, got, ref, S, bound):
    """both components against their own sums of absolute terms"""
    got, ref, S = np.asarray(got), np.asarray(ref, CLD), np.asarray(S, CLD)
    rep.cmp(what + " (re)", got.real, ref.real, bound(S.real))
    rep.cmp(what + " (im)", got.imag, ref.imag, bound(S.imag))


# ------------------------------------------------------------------------------------------------------------------
# layouts
# ------------------------------------------------------------------------------------------------------------------
def zlayout(dt, m, ncols, flavour, extra=0):
    """one complex panel operand; extra widens ld (not for 'eq') so that the operands of a case differ in it"""
    npdt = np.dtype(NPDT[dt])
    if flavour == "eq":
        return Operand(npdt, m, ncols, m, 0)
    if flavour == "odd":
        return Operand(npdt, m, ncols, (m + 1 if m % 2 == 0 else m + 2) + 2 * extra, 0)
    if flavour == "even":
        return Operand(npdt, m, ncols, (m + 2 if m % 2 == 0 else m + 1) + 2 * extra, 0)
    assert flavour == "shift" and dt == C32
    return Operand(npdt, m, ncols, m + 1 + extra, 1)


def zsmall(rows, ncols=1, spare=3):
    """(re, im) pairs of doubles: `rows` live pairs per column, `spare` NaN pairs behind them; ld counts pairs"""
    return Operand(np.complex128, rows, ncols, rows + spare, 0)


# ------------------------------------------------------------------------------------------------------------------
# references
# ------------------------------------------------------------------------------------------------------------------
def _c(x):
    return np.asarray(x, CLD)


def _rz(x, dt):
    """round to the panel type, back in clongdouble"""
    return _c(x).astype(NPDT[dt]).astype(CLD)


def absz(x):
    x = _c(x)
    return np.abs(x.real) + 1j * np.abs(x.imag)


def smul(Pm, SQ):
    """absolute terms of the components of Pm @ Q when the components of Q have the absolute terms SQ"""
    Pm, SQ = _c(Pm), _c(SQ)
    pr, pi = np.abs(Pm.real), np.abs(Pm.imag)
    return (pr @ SQ.real + pi @ SQ.imag) + 1j * (pr @ SQ.imag + pi @ SQ.real)


def sprod(p, SQ):
    """the same element by element"""
    p, SQ = _c(p), _c(SQ)
    pr, pi = np.abs(p.real), np.abs(p.imag)
    return (pr * SQ.real + pi * SQ.imag) + 1j * (pr * SQ.imag + pi * SQ.real)


def n2z(x):
    return (x.real * x.real + x.imag * x.imag).sum(axis=-1)


def ref_zdots(A, X):
    """out[c, j] = col_j^H X(:,c): the LEFT operand is conjugated"""
    A, X = _c(A), _c(X)
    return X @ A.conj().T, smul(X, absz(A).T)


def ref_zproject(dt, A, coef, X):
    """Xout(:,c) = X(:,c) - [segs] coef(:,c) with coef[c, j] (unconjugated); nrm2[c] = |Xout(:,c)|^2 as stored (real)"""
    A, X, coef = _c(A), _c(X), _c(coef)
    out = X - coef @ A
    S = absz(X) + smul(coef, absz(A))
    return out, S, n2z(_rz(out, dt)), n2z(S)


def ref_zproject_mul(A, coef, Mc, X):
    """X <- (X - [segs] coef) M with Mc[c, q] = M(q, c) = M[q + c nx]"""
    A, X, coef, Mc = _c(A), _c(X), _c(coef), _c(Mc)
    Y = X - coef @ A
    SY = absz(X) + smul(coef, absz(A))
    return Mc @ Y, smul(Mc, SY)


def ref_zritz(V, W, Hc, theta, kinds):
    """row q: V h_q (XV), W h_q (XW) or W h_q - theta_q V h_q (RES), h unconjugated, theta real"""
    V, W, Hc = _c(V), _c(W), _c(Hc)
    th = np.asarray(theta, LD)[:, None]
    xv, xw, sv, sw = Hc @ V, Hc @ W, smul(Hc, absz(V)), smul(Hc, absz(W))
    kinds = np.asarray(kinds)[:, None]
    out = np.where(kinds == XV, xv, np.where(kinds == XW, xw, xw - th * xv))
    S = np.where(kinds == XV, sv, np.where(kinds == XW, sw, sw + np.abs(th) * sv))
    return out, S


# ------------------------------------------------------------------------------------------------------------------
# the host dispatch of csrc/hipk_complex.hip, mirrored
# ------------------------------------------------------------------------------------------------------------------
def zdots_launches(nx, tot, mfma):
    """zpanel_dots_t: [(kernel, NX, CPW, nc)] per column chunk, or the one matrix-core launch"""
    if nx >= 4 and mfma:
        return [("zdots_mfma_kernel", 1 if tot <= 16 else 2)]
    want, out = (tot + 3) // 4, []
    for c0 in range(0, nx, 8):
        nc = nx - c0
        if nc == 1:
            NX, CPW = 1, 2 if want <= 2 else 4 if want <= 4 else 8 if want <= 8 else 16
        elif nc == 2:
            NX, CPW = 2, 2 if want <= 2 else 4 if want <= 4 else 8
        elif nc <= 4:
            NX, CPW = 4, 2 if want <= 2 else 4 if want <= 4 else 8
        else:
            NX, CPW = 8, 2 if want <= 2 else 4
        out.append(("zdots_kernel", NX, CPW, min(nc, 8)))
    return out


def zproject_launches(nx, tot, mul):
    """zproject_t: the return code when nothing is launched (1 not covered, -1 error), else [NXV per launch]"""
    if mul:
        nxm = 1 if nx <= 1 else 2 if nx <= 2 else 4 if nx <= 4 else 8
        return 1 if nx > 8 or tot * nxm > ZPROJ_LDS else [nxm]
    if tot > ZPROJ_LDS:
        return -1
    out, c0 = [], 0
    while c0 < nx:
        nc = nx - c0
        nxv = 4 if nc >= 4 else 2 if nc >= 2 else 1
        while nxv > 1 and tot * nxv > ZPROJ_LDS:
            nxv >>= 1
        out.append(nxv)
        c0 += nxv
    return out


ZRITZ2_FEW = [(2, 7, 7, 2), (2, 9, 7, 2), (2, 12, 10, 2), (4, 8, 7, 1)]      # tried in this order while nr <= 4
ZRITZ2_ANY = [(2, 4, 4, 8), (4, 8, 4, 4)]                                  # then these
ZRITZ1 = [(8, 4), (16, 4), (32, 4), (16, 16), (32, 16)]


def _count(jobs):
    nv = sum(1 for j in jobs if j[0] == XV)
    nw = sum(1 for j in jobs if j[0] == XW)
    return nv, nw, len(jobs) - nv - nw


def zritz_launch(jobs, allow_split, nosplit):
    """zritz_launch + zjobs_split's fit test: the instantiation one launch of these jobs runs, None if they fit no launch"""
    nv, nw, nr = _count(jobs)
    np_ = nv + nw
    if (np_ > 12 or nr > 4) and not (np_ == 0 and nr <= 16) and nr <= 16 and not nosplit and allow_split:
        for (L, a, b, c) in (ZRITZ2_FEW if nr <= 4 else []) + ZRITZ2_ANY:
            if -(-nv // L) <= a and -(-nw // L) <= b and -(-nr // L) <= c:
                return ("zritz2_kernel", L, a, b, c)
    if nr <= 4 and np_ <= 4:
        return ("zritz_kernel", 8, 4)
    if nr <= 4 and np_ <= 12:
        return ("zritz_kernel", 16, 4)
    if nr <= 4 and np_ <= 28:
        return ("zritz_kernel", 32, 4)
    if np_ == 0 and nr <= 16:
        return ("zritz_kernel", 16, 16)
    if nr <= 16 and np_ <= 16:
        return ("zritz_kernel", 32, 16)
    return None


def zritz_launches(jobs, nosplit=False):
    """zritz_t: the launches of a job list, in order (more than one = the chunked path through a temporary)"""
    one = zritz_launch(jobs, True, nosplit)
    if one is not None:
        return [one]
    out, chunk, cp, cr = [], [], 0, 0
    for q in range(len(jobs) + 1):
        res = q < len(jobs) and jobs[q][0] == RES
        if q == len(jobs) or (cr == 16 if res else cp == 16):
            if chunk:
                out.append(zritz_launch(chunk, False, nosplit))
            chunk, cp, cr = [], 0, 0
        if q < len(jobs):
            chunk.append(jobs[q])
            cr, cp = cr + res, cp + (not res)
    assert None not in out
    return out


def ritz_jt(inst):
    """columns of the coefficient block one LDS tile holds"""
    return 64 if inst[0] == "zritz_kernel" else 128 // inst[1]


def copy_path(c):
    """hipk_copy_cols (device allocations are 256-byte aligned, the guard is a multiple of 16 bytes)"""
    es = np.dtype(NPDT[c["dt"]]).itemsize
    nbytes = c["m"] * es
    if nbytes < COPY_MIN_BYTES:
        return ("memcpy2d",)
    v16 = (c["shift"] * es) % 16 == 0 and (c["nx"] == 1 or ((c["ldx"] * es) % 16 == 0 and (c["ldy"] * es) % 16 == 0))
    if v16:
        return ("lanes16", "left-over" if nbytes % 16 else "whole")
    return ("lanes%d" % (4 if es == 4 else 8),)


def branch_of(c, nosplit=False):
    """The instantiation(s) the documented dispatch sends a case to; a list where a call makes several launches.  THIS
    MIRRORS zpanel_dots_t, zproject_t, zritz_t / zritz_launch / zjobs_split of csrc/hipk_complex.hip and hipk_copy_cols of
    csrc/hipk_vec.hip: when the dispatch changes, this function and the tables change with it.  nosplit: HIPK_Z_NO_SPLIT."""
    ep, t = c["ep"], TNAME[c["dt"]]
    if ep == "dots":
        return [(x[0], t) + x[1:3] if x[0] == "zdots_kernel" else (x[0], t, x[1]) for x in zdots_launches(c["nx"], c["tot"], c.get("mfma", False))]
    if ep in ("project", "project_mul"):
        ln = zproject_launches(c["nx"], c["tot"], ep == "project_mul")
        return ln if isinstance(ln, int) else [("zproject_kernel", t, nxv, ep == "project_mul") for nxv in ln]
    if ep == "ritz_update":
        return [(x[0], t) + x[1:] for x in zritz_launches(c["jobs"], nosplit)]
    if ep == "copy_cols":
        return [("copy_cols", t) + copy_path(c)]
    if ep == "columns":
        return [(c["op"], t)]
    raise ValueError(ep)


PASS_ROWS = {"dots": 64, "project": 256, "project_mul": 256, "columns": 256, "copy_cols": 256}


def size_of(c, inst=None):
    """'s' below the rows one workgroup takes per pass, 'l' above and not a multiple of it, 'x' an exact multiple"""
    rows = PASS_ROWS.get(c["ep"])
    if c["ep"] == "ritz_update":
        rows = 256 if inst[0] == "zritz_kernel" else 256 // inst[2]
    return "s" if c["m"] < rows else "l" if c["m"] % rows else "x"


# ------------------------------------------------------------------------------------------------------------------
# case tables (static)
# ------------------------------------------------------------------------------------------------------------------
ROWS = [1, 2, 63, 64, 65, 127, 128, 129, 255, 256, 257, 700, 1999]
M64_S, M64_L = [1, 2, 63], [257, 65, 700, 129, 1999, 127, 255]            # against 64 rows per pass
M256_S, M256_L = [1, 63, 65, 2, 127, 129, 255, 64, 128], [257, 700, 1999]  # against 256 rows per pass
MX = [64, 128, 256]


class _Rot:
    def __init__(self):
        self.i = 0

    def next(self, seq):
        self.i += 1
        return seq[(self.i - 1) % len(seq)]


def _fl(dt, n):
    return FLAVOURS[dt][n % len(FLAVOURS[dt])]


# tot per CPW of zdots_kernel: [a multiple of 4 CPW, a whole wave idle (j0 >= tot), ragged], then what gives blockIdx.y > 0
DOTS_TOT = {(1, 2): [8, 5, 3], (1, 4): [16, 9, 15], (1, 8): [32, 17, 27], (1, 16): [64, 33, 65, 130],
            (2, 2): [8, 5, 1], (2, 4): [16, 9, 14], (2, 8): [32, 17, 70, 64],
            (4, 2): [8, 5, 7], (4, 4): [16, 9, 13], (4, 8): [32, 17, 70, 64],
            (8, 2): [8, 5, 2], (8, 4): [16, 9, 33, 48]}
DOTS_NX = {1: [1, 9], 2: [2, 10], 4: [4, 3, 11, 12], 8: [8, 5, 6, 7, 13]}


def _dots_cases():
    out, rs, rl, n = [], _Rot(), _Rot(), 0
    for dt in ZTYPES:
        for (NX, CPW), tots in DOTS_TOT.items():
            for ti, tot in enumerate(tots):
                for ni, nx in enumerate(DOTS_NX[NX]):
                    n += 1
                    big = (ti + ni) % 2 == 1
                    split = 1 + (n % 3)
                    xseg = n % 5 == 0 and tot >= 2
                    out.append(dict(ep="dots", dt=dt, m=rl.next(M64_L) if big else rs.next(M64_S), nx=nx, tot=tot, split=min(split, 2) if xseg else split,
                                    xseg=xseg, ldout=["eq", "gt"][(n // 2) % 2], flavour=_fl(dt, n), mfma=False))
        for i, m in enumerate(MX):        # exact multiples of the rows of one pass
            out.append(dict(ep="dots", dt=dt, m=m, nx=[3, 8, 1][i], tot=[9, 5, 40][i], split=1 + i, xseg=False, ldout=["eq", "gt"][i % 2],
                            flavour=_fl(dt, i), mfma=False))
    return out


MFMA_NX = [4, 5, 8, 9, 11, 16]
MFMA_TOT = [1, 15, 16, 17, 31, 33, 48, 70]
MFMA_HALVING = dict(m=1999, tot=300, nx=25)       # gm gy gz = 32 * 10 * 4 > 256 CUs * 2 * 2


def _dots_mfma_cases():
    out, rs, rl, n = [], _Rot(), _Rot(), 0
    for dt in ZTYPES:
        for ni, nx in enumerate(MFMA_NX):
            for ti, tot in enumerate(MFMA_TOT):
                n += 1
                big = (ti + ni) % 2 == 1
                split = 1 + (n % 3)
                xseg = n % 7 == 0 and tot >= 2
                out.append(dict(ep="dots", dt=dt, m=rl.next(M64_L) if big else rs.next(M64_S), nx=nx, tot=tot, split=min(split, 2) if xseg else split,
                                xseg=xseg, ldout=["eq", "gt"][(n // 2) % 2], flavour=_fl(dt, n), mfma=True))
        for i, nx in enumerate((1, 2, 3)):          # the switch on, fewer than four columns: the vector-unit kernel
            out.append(dict(ep="dots", dt=dt, m=[63, 257, 700][i], nx=nx, tot=[17, 5, 33][i], split=1 + i, xseg=False, ldout=["gt", "eq"][i % 2],
                            flavour=_fl(dt, i), mfma=True))
        out.append(dict(ep="dots", dt=dt, split=2, xseg=False, ldout="eq", flavour="odd", mfma=True, halving=True, **MFMA_HALVING))
    return out


def mfma_halves(c, num_cu, mbpc=2):
    """does zpanel_dots_t's loop `while (gm > 1 && gm gy gz > num_cu 2 mbpc)` run at least once for this case"""
    need = max((c["m"] + 63) // 64, 1)
    nt = 1 if c["tot"] <= 16 else 2
    gy, gz = -(-c["tot"] // (16 * nt)), (c["nx"] + 7) // 8
    gm = min(need, num_cu * mbpc)
    return gm > 1 and gm * gy * gz > num_cu * 2 * mbpc


PROJECT_NX = [1, 2, 3, 4, 5, 6, 7, 9]
PROJECT_TOT = [1, 8, 37, 0]
PROJECT_BIGTOT = [512, 513, 1024, 1025, 2048]
PLACES = ["in", "out", "alias"]                   # hipk_panel_project; hipk_panel_project_to; the latter with Xout == X


def _project_cases():
    out, rs, rl, n = [], _Rot(), _Rot(), 0
    for dt in ZTYPES:
        for ni, nx in enumerate(PROJECT_NX):
            for si in range(2):
                for rep in range(2):
                    n += 1
                    out.append(dict(ep="project", dt=dt, m=rl.next(M256_L) if si else rs.next(M256_S), nx=nx, tot=PROJECT_TOT[(ni + si + 2 * rep) % 4],
                                    split=1 + (n % 3), norms=(n // 2) % 2 == 0, place=PLACES[n % 3], flavour=_fl(dt, n)))
        for ti, tot in enumerate(PROJECT_BIGTOT):   # the LDS-driven halvings of the column chunk, at a tiny m
            for ni, nx in enumerate((4, 7)):
                n += 1
                out.append(dict(ep="project", dt=dt, m=[63, 65, 2, 64, 1][(ti + ni) % 5], nx=nx, tot=tot, split=1 + (n % 3), norms=n % 2 == 0,
                                place=PLACES[n % 3], flavour=_fl(dt, n)))
        for pi, place in enumerate(PLACES):          # one column too many: -1, nothing written
            out.append(dict(ep="project", dt=dt, m=[2, 63, 1][pi], nx=[1, 4, 2][pi], tot=2049, split=1 + pi, norms=pi != 1, place=place, flavour=_fl(dt, pi)))
        for i, m in enumerate(MX):
            out.append(dict(ep="project", dt=dt, m=m, nx=[7, 2, 5][i], tot=[8, 37, 1][i], split=1 + i, norms=True, place=PLACES[i], flavour=_fl(dt, i)))
    return out


MUL_EDGE = [(8, 256), (8, 257), (5, 256), (5, 257), (4, 512), (4, 513), (3, 512), (3, 513), (2, 1024), (2, 1025), (1, 2048), (1, 2049)]


def _project_mul_cases():
    out, rs, rl, n = [], _Rot(), _Rot(), 0
    for dt in ZTYPES:
        for nx in range(1, 9):
            for ti, tot in enumerate((0, 1, 24)):
                for si in range(2):
                    n += 1
                    if ti == 0 and si != nx % 2:
                        continue
                    out.append(dict(ep="project_mul", dt=dt, m=rl.next(M256_L) if si else rs.next(M256_S), nx=nx, tot=tot, split=1 + (n % 3), flavour=_fl(dt, n)))
        for i, (nx, tot) in enumerate(MUL_EDGE):     # tot * NXV just below / above the LDS limit: above it 1, nothing written
            out.append(dict(ep="project_mul", dt=dt, m=[63, 2, 65, 1][i % 4], nx=nx, tot=tot, split=2, flavour=_fl(dt, i)))
        for i in range(2):
            out.append(dict(ep="project_mul", dt=dt, m=[63, 257][i], nx=9, tot=[3, 0][i], split=2, flavour=_fl(dt, i)))
        out.append(dict(ep="project_mul", dt=dt, m=256, nx=6, tot=10, split=3, flavour=_fl(dt, 1)))
    return out


RITZ_NH = 8
# (V-products, W-products, residuals) that fit the form and nothing tried before it
RITZ_MIX = {("zritz_kernel", 8, 4): (2, 1, 2), ("zritz_kernel", 16, 4): (5, 4, 3), ("zritz_kernel", 16, 16): (0, 0, 7),
            ("zritz2_kernel", 2, 7, 7, 2): (8, 6, 3), ("zritz2_kernel", 2, 9, 7, 2): (17, 5, 4), ("zritz2_kernel", 2, 12, 10, 2): (20, 16, 2),
            ("zritz2_kernel", 4, 8, 7, 1): (26, 22, 4), ("zritz2_kernel", 2, 4, 4, 8): (8, 3, 5), ("zritz2_kernel", 4, 8, 4, 4): (11, 5, 6)}
# job lists that fit no single launch -> the chunked path; <32, 4> and <32, 16> are reachable only here
RITZ_CHUNKED = [(34, 3, 6), (2, 0, 18)]


def _ritz_jobs(k, nv, nw, nr):
    """XV / XW in place on the first columns and into the third panel E; residuals into spare columns of W, into E, or
    nowhere (dst NULL, slot only); the third residual has a destination and slot -1"""
    jobs, e, slot = [], 0, 0
    for c in range(nv):
        if c < min(k, 3):
            jobs.append((XV, c % RITZ_NH, ("V", c), -1))
        else:
            jobs.append((XV, c % RITZ_NH, ("E", e), -1)); e += 1
    for c in range(nw):
        if c < min(k, 2):
            jobs.append((XW, (c + 2) % RITZ_NH, ("W", c), -1))
        else:
            jobs.append((XW, (c + 2) % RITZ_NH, ("E", e), -1)); e += 1
    for r in range(nr):
        if r % 3 == 1:
            dst = None
        elif r % 3 == 0:
            dst = ("W", k + r)
        else:
            dst = ("E", e); e += 1
        if nr >= 3 and r == 2:
            jobs.append((RES, (r + 1) % RITZ_NH, dst, -1))
        else:
            jobs.append((RES, (r + 1) % RITZ_NH, dst, slot)); slot += 1
    return jobs, max(e, 1)


def _ritz_update_cases():
    out, n = [], 0
    for dt in ZTYPES:
        for inst, (nv, nw, nr) in RITZ_MIX.items():
            jt = ritz_jt(inst)
            for ki, k in enumerate((jt, jt + 1)):          # staged once; in two tiles
                for si in range(2):
                    n += 1
                    jobs, ne = _ritz_jobs(k, nv, nw, nr)
                    out.append(dict(ep="ritz_update", dt=dt, m=[M64_S, M256_L][si][(n // 2) % 3], k=k, jobs=jobs, necols=ne, flavour=_fl(dt, n)))
            n += 1
            jobs, ne = _ritz_jobs(3, nv, nw, nr)
            out.append(dict(ep="ritz_update", dt=dt, m=MX[n % 3], k=3, jobs=jobs, necols=ne, flavour=_fl(dt, n)))
        for ci, (nv, nw, nr) in enumerate(RITZ_CHUNKED):
            for ki, k in enumerate((64, 65)):
                for si in range(2):
                    n += 1
                    jobs, ne = _ritz_jobs(k, nv, nw, nr)
                    out.append(dict(ep="ritz_update", dt=dt, m=[M64_S, M256_L][si][(n // 2) % 3], k=k, jobs=jobs, necols=ne, flavour=_fl(dt, n)))
    return out


COL_OPS = {"axpy": [1, 3, 64, 65], "xpay": [1, 3, 64, 65], "pair_dots": [1, 3, 8], "scale": [3, 65], "rsqrt": [1, 3], "norms2": [1, 3],
           "residual": [3, 65], "gather": [3, 65]}


def _columns_cases():
    out, n = [], 0
    for dt in ZTYPES:
        for op, nxs in COL_OPS.items():
            for ni, nx in enumerate(nxs):
                for si in range(2):
                    n += 1
                    m = (M256_L if nx < 64 else [257, 700])[n % (3 if nx < 64 else 2)] if si else M256_S[n % len(M256_S)]
                    out.append(dict(ep="columns", op=op, dt=dt, m=m, nx=nx, flavour=_fl(dt, n)))
            out.append(dict(ep="columns", op=op, dt=dt, m=256, nx=nxs[0], flavour=_fl(dt, n)))
    return out


def _copy_cases():
    """the thresholds of hipk_copy_cols are in BYTES: the row counts are 4096 / (element size) - 1 (2-D copy), that number
    (the first lane-copied size, a whole number of 16-byte lanes) and 1999 (bytes left over for all types but C64)"""
    out = []
    for dt in (F64, F32, C64, C32):
        es = np.dtype(NPDT[dt]).itemsize
        w, at = 16 // es, COPY_MIN_BYTES // es

        def up(v):
            return -(-v // w) * w

        def odd(v):
            return v + 1 if v % 2 == 0 else v + 2
        out.append(dict(ep="copy_cols", dt=dt, m=at - 1, nx=3, ldx=odd(at), ldy=at + 5, shift=0))
        out.append(dict(ep="copy_cols", dt=dt, m=63, nx=2, ldx=63, ldy=64, shift=1))
        out.append(dict(ep="copy_cols", dt=dt, m=at, nx=3, ldx=at, ldy=at + 2 * w, shift=0))
        out.append(dict(ep="copy_cols", dt=dt, m=1999, nx=3, ldx=up(1999) + w, ldy=up(1999), shift=0))
        out.append(dict(ep="copy_cols", dt=dt, m=1999, nx=3, ldx=odd(1999), ldy=odd(1999) + 2, shift=0))
        out.append(dict(ep="copy_cols", dt=dt, m=at, nx=3, ldx=up(at) + w, ldy=up(at) + 2 * w, shift=1))
        out.append(dict(ep="copy_cols", dt=dt, m=1999, nx=1, ldx=odd(1999), ldy=odd(1999) + 2, shift=0))
        out.append(dict(ep="copy_cols", dt=dt, m=at + 1, nx=1, ldx=at + 1, ldy=at + 1, shift=1))
    return out


CASES = {"dots": _dots_cases(), "dots_mfma": _dots_mfma_cases(), "project": _project_cases(), "project_mul": _project_mul_cases(),
         "ritz_update": _ritz_update_cases(), "columns": _columns_cases(), "copy_cols": _copy_cases()}
TABLES = list(CASES)

# Cases the plain-C oracle cannot run as they are, by name and with the reason (nothing is skipped silently):
ORACLE_CANNOT = {
    "dots_mfma": "hipk_set_zdots_mfma selects between device kernels; the oracle has one loop (the same shapes run on it as plain dots cases)",
}


def case_id(c):
    keys = [k for k in ("op", "m", "k", "nx", "tot", "split", "xseg", "ldout", "norms", "place", "ldx", "ldy", "shift", "flavour", "mfma") if k in c]
    s = ",".join(f"{k}={c[k]}" for k in keys)
    if "jobs" in c:
        s += ",jobs=%d+%d+%d" % _count(c["jobs"])
    return f"{c['ep']}[{TNAME[c['dt']]},{s}]"


# ------------------------------------------------------------------------------------------------------------------
# cells: what a case covers, and what a table has to cover
# ------------------------------------------------------------------------------------------------------------------
def _dots_marks(NX, CPW, nc, tot):
    last = tot - (-(-tot // (4 * CPW)) - 1) * 4 * CPW           # columns of the last blockIdx.y group
    marks = ["full" if tot % (4 * CPW) == 0 else "ragged", "nxv=NX" if nc == NX else "nxv<NX"]
    if last <= 3 * CPW:
        marks.append("idle-wave")
    if tot > 4 * CPW:
        marks.append("multi-y")
    return marks


def cells_of(c, nosplit=False):
    ep, t = c["ep"], TNAME[c["dt"]]
    b = branch_of(c, nosplit)
    if ep == "dots":
        cells = {("split", t, c["split"]), ("ldout", t, c["ldout"])} | ({("xseg", t)} if c["xseg"] else set())
        if b[0][0] == "zdots_mfma_kernel":
            cells |= {("inst",) + b[0], ("nx", t, c["nx"]), ("tot", t, c["tot"])} | ({("halving", t)} if c.get("halving") else set())
            return cells
        if c["mfma"]:
            cells.add(("fallthrough", t, c["nx"]))
        for i, x in enumerate(zdots_launches(c["nx"], c["tot"], False)):
            inst = ("inst", x[0], t, x[1], x[2])
            cells.add(inst)
            cells |= {inst + (mk,) for mk in _dots_marks(x[1], x[2], x[3], c["tot"])}
            if i > 0:
                cells.add(("chunk2", t, c["nx"]))
        return cells
    if ep in ("project", "project_mul"):
        cells = {("nx", t, c["nx"]), ("tot", t, c["tot"]), ("split", t, c["split"])}
        if ep == "project":
            cells |= {("norms", t, c["norms"]), ("place", t, c["place"])}
        if isinstance(b, int):
            return cells | {("rc", t, b, c["nx"], c["tot"])}
        return cells | {("inst",) + x for x in b} | ({("edge", t, c["nx"], c["tot"])} if ep == "project_mul" else set())
    if ep == "ritz_update":
        cells = set()
        for x in b:
            cells |= {("inst",) + x, ("inst",) + x + ("once" if c["k"] <= ritz_jt(x[:1] + x[2:]) else "tiled",)}
        if len(b) > 1:
            cells.add(("chunked", t, _count(c["jobs"])))
        return cells
    if ep == "columns":
        return {("inst",) + b[0], ("nx", t, c["op"], c["nx"])}
    if ep == "copy_cols":
        return {("inst",) + b[0], ("nx", t, c["nx"])} | ({("nx1-unaligned-stride", t)} if c["nx"] == 1 and b[0][2] == "lanes16" and c["shift"] == 0 else set()) \
            | ({("lanes", t, "shift" if c["shift"] else "ld")} if b[0][2] in ("lanes4", "lanes8") else set())
    raise ValueError(ep)


ZDOTS_INST = sorted(DOTS_TOT)


def wanted_cells(table, nosplit=False):
    want = set()
    for t in ("c64", "c32"):
        if table == "dots":
            for (NX, CPW) in ZDOTS_INST:
                inst = ("inst", "zdots_kernel", t, NX, CPW)
                want |= {inst, inst + ("full",), inst + ("ragged",), inst + ("idle-wave",), inst + ("nxv=NX",)}
                if NX >= 4:
                    want.add(inst + ("nxv<NX",))
                if (NX, CPW) in ((1, 16), (2, 8), (4, 8), (8, 4)):      # the others end at tot = 4 CPW
                    want.add(inst + ("multi-y",))
            want |= {("chunk2", t, nx) for nx in (9, 11)} | {("split", t, s) for s in (1, 2, 3)} | {("xseg", t)} | {("ldout", t, x) for x in ("eq", "gt")}
        elif table == "dots_mfma":
            want |= {("inst", "zdots_mfma_kernel", t, nt) for nt in (1, 2)} | {("nx", t, nx) for nx in MFMA_NX} | {("tot", t, tot) for tot in MFMA_TOT}
            want |= {("fallthrough", t, nx) for nx in (1, 2, 3)} | {("ldout", t, x) for x in ("eq", "gt")} | {("halving", t)}
        elif table == "project":
            want |= {("inst", "zproject_kernel", t, nxv, False) for nxv in (1, 2, 4)} | {("nx", t, nx) for nx in PROJECT_NX}
            want |= {("tot", t, tot) for tot in PROJECT_TOT + PROJECT_BIGTOT} | {("norms", t, b) for b in (True, False)} | {("place", t, p) for p in PLACES}
            want |= {("split", t, s) for s in (1, 2, 3)} | {("rc", t, -1, nx, 2049) for nx in (1, 4, 2)}
        elif table == "project_mul":
            want |= {("inst", "zproject_kernel", t, nxv, True) for nxv in (1, 2, 4, 8)} | {("nx", t, nx) for nx in range(1, 10)} | {("tot", t, 0)}
            want |= {("edge", t, nx, tot) for (nx, tot) in MUL_EDGE[0::2]} | {("rc", t, 1, nx, tot) for (nx, tot) in MUL_EDGE[1::2]}
            want |= {("rc", t, 1, 9, 3), ("rc", t, 1, 9, 0)}
        elif table == "ritz_update":
            forms = [x for x in ZRITZ1] if nosplit else ZRITZ1 + ZRITZ2_FEW + ZRITZ2_ANY
            for f in forms:
                inst = ("inst", "zritz_kernel" if len(f) == 2 else "zritz2_kernel", t) + f
                want |= {inst, inst + ("once",), inst + ("tiled",)}
            want |= {("chunked", t, mix) for mix in RITZ_CHUNKED}
        elif table == "columns":
            want |= {("inst", op, t) for op in COL_OPS} | {("nx", t, op, nx) for op, nxs in COL_OPS.items() for nx in nxs}
    if table == "copy_cols":
        for t in ("f64", "f32", "c64", "c32"):
            want |= {("inst", "copy_cols", t, "memcpy2d"), ("inst", "copy_cols", t, "lanes16", "whole"), ("nx", t, 1), ("nx", t, 3)}
            if t != "c64":      # a complex double is 16 bytes: no column of it leaves bytes over or loses the alignment
                want |= {("inst", "copy_cols", t, "lanes16", "left-over"), ("inst", "copy_cols", t, "lanes4" if t == "f32" else "lanes8"),
                         ("lanes", t, "shift"), ("lanes", t, "ld"), ("nx1-unaligned-stride", t)}
    return want


def coverage(table, nosplit=False):
    """(cells covered, cells wanted, instantiations that lack a row count below one pass or one that is no multiple of it)"""
    have, sizes = set(), {}
    for c in CASES[table]:
        cells = cells_of(c, nosplit)
        have |= cells
        for x in cells:
            if x[0] == "inst" and x[-1] not in ("once", "tiled", "full", "ragged", "idle-wave", "nxv=NX", "nxv<NX", "multi-y"):
                sizes.setdefault(x, set()).add(size_of(c, x[1:]))
    want = wanted_cells(table, nosplit)
    one_size = sorted(str(b) for b, s in sizes.items() if b in want and not {"s", "l"} <= s)
    if table == "copy_cols":
        one_size = []            # its paths are chosen by the BYTES of a column: see _copy_cases
    return have, want, one_size


def instantiations(table):
    """the template instantiations among the wanted cells (without the refinements)"""
    marks = ("once", "tiled", "full", "ragged", "idle-wave", "nxv=NX", "nxv<NX", "multi-y")
    return {x for x in wanted_cells(table) if x[0] == "inst" and x[-1] not in marks}


# ------------------------------------------------------------------------------------------------------------------
# runners
# ------------------------------------------------------------------------------------------------------------------
def _rng(c):
    return np.random.default_rng(zlib.crc32(case_id(c).encode()))


def _zrand(rng, shape, dt, scale=None):
    z = rng.standard_normal(shape) + 1j * rng.standard_normal(shape)
    if scale is not None:
        z = z * scale
    return z.astype(NPDT[dt])


def _make_segs(c, rng, dt, m, tot, Xop=None, Xd=None):
    """the basis columns over 1..3 segment operands (an empty segment still has a valid base), a different magnitude per
    column; with Xop the LAST segment is column 0 of the right-hand panel itself"""
    A = _zrand(rng, (tot, m), dt, np.linspace(0.5, 2.0, max(tot, 1))[:tot, None])
    counts = P._split(tot, c["split"])
    if Xop is not None:
        counts = P._split(tot - 1, c["split"]) + [1]
        A[tot - 1] = Xd[0]
    ops, j = [], 0
    for s, n in enumerate(counts):
        if Xop is not None and s == len(counts) - 1:
            ops.append((Xop, 1))
        else:
            op = zlayout(dt, m, max(n, 1), c["flavour"], extra=1 + s % 2)
            if n:
                op.fill(range(n), A[j:j + n])
            ops.append((op, n))
        j += n
    return ops, A


def _upload(side, ops, known=()):
    """one device array per distinct operand"""
    tens = {id(op): t for op, t in known}
    for op in ops:
        if id(op) not in tens:
            tens[id(op)] = side.arr(op.host)
    return tens


def _check_guards(side, rep, cid, named, tens):
    got, seen = {}, set()
    for name, op in named:
        if id(op) in seen:
            continue
        seen.add(id(op))
        a = side.get(tens[id(op)])
        rep.guard(f"{cid} {name}", op, a)
        got[id(op)] = a
    return got


def _segs_arg(side, segs, tens):
    return P._seg_array(side, segs, [tens[id(op)] for op, _ in segs])


def _run_dots(side, c, rep):
    dt, m, nx, tot = c["dt"], c["m"], c["nx"], c["tot"]
    cid, rng = case_id(c), _rng(c)
    Xd = _zrand(rng, (nx, m), dt, np.linspace(1.0, 3.0, nx)[:, None])
    X = zlayout(dt, m, nx, c["flavour"])
    X.fill(range(nx), Xd)
    segs, A = _make_segs(c, rng, dt, m, tot, X if c["xseg"] else None, Xd)
    ref, S = ref_zdots(A, Xd)
    switch = c["mfma"] and hasattr(side.lib, "hipk_set_zdots_mfma")          # the oracle has no such switch: ORACLE_CANNOT
    res = []
    for form in ((1, 0) if switch else (None,)):
        out = zsmall(tot, nx, spare=0 if c["ldout"] == "eq" else 3)
        out.expect(range(nx))
        tens = _upload(side, [op for op, _ in segs] + [X, out])
        old = side.lib.hipk_set_zdots_mfma(form) if form is not None else None
        try:
            rc = side.lib.hipk_panel_dots(side.ctx, dt, m, _segs_arg(side, segs, tens), len(segs), X.base(side, tens[id(X)]), X.ld, nx,
                                          out.base(side, tens[id(out)]), out.ld)
            assert rc == 0, f"{cid}: rc = {rc}"
            got = _check_guards(side, rep, cid, [(f"seg{i}", op) for i, (op, _) in enumerate(segs)] + [("X", X), ("out", out)], tens)
        finally:
            if form is not None:
                side.lib.hipk_set_zdots_mfma(old)
        res.append(out.take(got[id(out)], range(nx)))
        zcmp(rep, f"{cid} out" + ("" if form is None else [" (vector units)", " (matrix cores)"][form]), res[-1], ref, S, lambda s: zbound_red(m, s))
    if switch and nx >= 4:
        # both forms are within one bound of the reference, so within two of each other
        zcmp(rep, f"{cid} matrix cores against vector units", res[0], res[1], S, lambda s: 2.0 * zbound_red(m, s))


def _run_project(side, c, rep):
    dt, m, nx, tot, place = c["dt"], c["m"], c["nx"], c["tot"], c["place"]
    cid, rng = case_id(c), _rng(c)
    want_rc = -1 if tot > ZPROJ_LDS else 0
    segs, A = _make_segs(c, rng, dt, m, tot)
    Xd = _zrand(rng, (nx, m), dt, np.linspace(1.0, 2.0, nx)[:, None])
    cf = (rng.standard_normal((nx, tot)) + 1j * rng.standard_normal((nx, tot))) / np.sqrt(max(tot, 1))
    X = zlayout(dt, m, nx, c["flavour"])
    X.fill(range(nx), Xd)
    O = zlayout(dt, m, nx, c["flavour"], extra=2) if place == "out" else X
    coef, n2 = zsmall(tot, nx), small(nx)
    if tot:
        coef.fill(range(nx), cf)
    if want_rc == 0:
        O.expect(range(nx))
        if c["norms"]:
            n2.expect(0)
    tens = _upload(side, [op for op, _ in segs] + [X, O, coef, n2])
    nptr = n2.base(side, tens[id(n2)]) if c["norms"] else None
    sa = _segs_arg(side, segs, tens)
    if place == "in":
        rc = side.lib.hipk_panel_project(side.ctx, dt, m, sa, len(segs), coef.base(side, tens[id(coef)]), coef.ld, X.base(side, tens[id(X)]), X.ld, nx, nptr)
    else:
        rc = side.lib.hipk_panel_project_to(side.ctx, dt, m, sa, len(segs), coef.base(side, tens[id(coef)]), coef.ld, X.base(side, tens[id(X)]), X.ld,
                                            O.base(side, tens[id(O)]), O.ld, nx, nptr)
    assert rc == want_rc, f"{cid}: rc = {rc}, the header says {want_rc}"
    got = _check_guards(side, rep, cid, [(f"seg{i}", op) for i, (op, _) in enumerate(segs)] + [("X", X), ("Xout", O), ("coef", coef), ("nrm2", n2)], tens)
    if want_rc:
        return
    ref, S, nref, Sn = ref_zproject(dt, A, cf, Xd)
    zcmp(rep, f"{cid} Xout", O.take(got[id(O)], range(nx)), ref, S, lambda s: zbound_elem(dt, tot, s))
    if c["norms"]:
        rep.cmp(f"{cid} nrm2", n2.take(got[id(n2)], 0)[0], nref, zbound_red(m, Sn, dt, tot))


def _run_project_mul(side, c, rep):
    dt, m, nx, tot = c["dt"], c["m"], c["nx"], c["tot"]
    cid, rng = case_id(c), _rng(c)
    ln = zproject_launches(nx, tot, True)
    want_rc = ln if isinstance(ln, int) else 0
    segs, A = _make_segs(c, rng, dt, m, tot)           # split 2: [Q | V]
    Xd = _zrand(rng, (nx, m), dt, np.linspace(1.0, 2.0, nx)[:, None])
    cf = (rng.standard_normal((nx, tot)) + 1j * rng.standard_normal((nx, tot))) / np.sqrt(max(tot, 1))
    Mc = (rng.standard_normal((nx, nx)) + 1j * rng.standard_normal((nx, nx))) / np.sqrt(nx)          # not Hermitian
    X, coef, Mo = zlayout(dt, m, nx, c["flavour"]), zsmall(max(tot, 1), nx), Operand(np.complex128, nx, nx, nx)
    X.fill(range(nx), Xd)
    if tot:
        coef.host[coef.index(range(nx), tot)] = cf
    Mo.fill(range(nx), Mc)
    if want_rc == 0:
        X.expect(range(nx))
    tens = _upload(side, [op for op, _ in segs] + [X, coef, Mo])
    rc = side.lib.hipk_panel_project_mul(side.ctx, dt, m, _segs_arg(side, segs, tens), len(segs), coef.base(side, tens[id(coef)]), coef.ld,
                                         Mo.base(side, tens[id(Mo)]), X.base(side, tens[id(X)]), X.ld, nx)
    assert rc == want_rc, f"{cid}: rc = {rc}, the header says {want_rc}"
    got = _check_guards(side, rep, cid, [(f"seg{i}", op) for i, (op, _) in enumerate(segs)] + [("coef", coef), ("M", Mo), ("X", X)], tens)
    if want_rc:
        return
    ref, S = ref_zproject_mul(A, cf, Mc, Xd)
    zcmp(rep, f"{cid} X", X.take(got[id(X)], range(nx)), ref, S, lambda s: zbound_elem(dt, tot + nx, s))


def _run_ritz_update(side, c, rep):
    dt, m, k, jobs = c["dt"], c["m"], c["k"], c["jobs"]
    cid, rng = case_id(c), _rng(c)
    Vd, Wd = _zrand(rng, (k, m), dt, np.linspace(0.5, 2.0, k)[:, None]), _zrand(rng, (k, m), dt, np.linspace(2.0, 0.5, k)[:, None])
    hc = (rng.standard_normal((RITZ_NH, k)) + 1j * rng.standard_normal((RITZ_NH, k))) / np.sqrt(k)
    theta = np.linspace(-1.3, 2.1, RITZ_NH) + 0.01 * rng.standard_normal(RITZ_NH)            # distinct per column
    nwx = max([d[1] + 1 for (_, _, d, _) in jobs if d and d[0] == "W"] + [k])
    nslots = max([s for (_, _, _, s) in jobs] + [-1]) + 1
    V, W, E = zlayout(dt, m, k, c["flavour"]), zlayout(dt, m, nwx, c["flavour"]), zlayout(dt, m, c["necols"], c["flavour"], extra=1)
    assert V.ld == W.ld                                     # V and W share one leading dimension
    V.fill(range(k), Vd); W.fill(range(k), Wd)
    where_op = {"V": V, "W": W, "E": E}
    for (_, _, d, _) in jobs:
        if d:
            where_op[d[0]].expect(d[1])
    H, TH, N2 = zsmall(k, RITZ_NH, spare=1), small(RITZ_NH), small(max(nslots, 1))
    H.fill(range(RITZ_NH), hc); TH.fill(0, theta)
    if nslots:
        N2.written[N2.index(0, nslots)] = True
    tens = _upload(side, [V, W, E, H, TH, N2])
    arr = P._jobs_array(side, jobs, {n: (op, tens[id(op)]) for n, op in where_op.items()})
    rc = side.lib.hipk_ritz_update(side.ctx, dt, m, V.base(side, tens[id(V)]), W.base(side, tens[id(W)]), V.ld, k, H.base(side, tens[id(H)]), H.ld,
                                   TH.base(side, tens[id(TH)]), arr, len(jobs), N2.base(side, tens[id(N2)]))
    assert rc == 0, f"{cid}: rc = {rc}"
    got = _check_guards(side, rep, cid, [("V", V), ("W", W), ("E", E), ("h", H), ("theta", TH), ("nrm2", N2)], tens)
    # from the ORIGINAL panels: the reads of a row precede its writes, whatever the destinations alias
    ref, S = ref_zritz(Vd, Wd, hc[[j[1] for j in jobs]], theta[[j[1] for j in jobs]], [j[0] for j in jobs])
    for q, (kind, col, d, slot) in enumerate(jobs):
        n = 2 * k if kind == RES else k
        if d:
            zcmp(rep, f"{cid} job {q} -> {d[0]}[{d[1]}]", where_op[d[0]].take(got[id(where_op[d[0]])], d[1])[0], ref[q], S[q], lambda s: zbound_elem(dt, n, s))
        if kind == RES and slot >= 0:
            rep.cmp(f"{cid} job {q} nrm2[{slot}]", got[id(N2)][N2.off + slot], n2z(_rz(ref[q], dt)), zbound_red(m, n2z(S[q]), dt, n))


def _dp(a):
    return a.ctypes.data_as(C.POINTER(C.c_double))


def _run_columns(side, c, rep):
    dt, m, nx, op = c["dt"], c["m"], c["nx"], c["op"]
    cid, rng = case_id(c), _rng(c)
    Xd = _zrand(rng, (nx, m), dt, np.linspace(1.0, 2.0, nx)[:, None])
    Yd = _zrand(rng, (nx, m), dt, np.linspace(2.0, 0.7, nx)[:, None])
    X, Y = zlayout(dt, m, nx, c["flavour"], extra=1), zlayout(dt, m, nx, c["flavour"], extra=2)
    X.fill(range(nx), Xd); Y.fill(range(nx), Yd)
    a = np.ascontiguousarray(rng.standard_normal(nx) + 1j * rng.standard_normal(nx))
    r = np.ascontiguousarray(np.linspace(-1.5, 2.5, nx) + 0.01 * rng.standard_normal(nx))       # real factors, distinct per column
    xl, yl, al, rl = _c(Xd), _c(Yd), _c(a)[:, None], np.asarray(r, LD)[:, None]
    dres = zsmall(nx) if op == "pair_dots" else small(nx)
    if op in ("pair_dots", "norms2", "residual"):
        dres.expect(0)
    if op == "rsqrt":
        dres.fill(0, np.linspace(0.3, 4.0, nx))
    if op != "pair_dots" and op != "norms2":
        Y.expect(range(nx))
    perm = [(7 * i + nx // 2) % nx for i in range(nx)]
    tens = _upload(side, [X, Y, dres])
    xp, yp, dp = X.base(side, tens[id(X)]), Y.base(side, tens[id(Y)]), dres.base(side, tens[id(dres)])
    L = side.lib
    if op == "axpy":
        rc = L.hipk_axpy_cols(side.ctx, dt, m, _dp(a.view(np.float64)), xp, X.ld, yp, Y.ld, nx)
    elif op == "xpay":
        rc = L.hipk_xpay_cols(side.ctx, dt, m, _dp(a.view(np.float64)), xp, X.ld, yp, Y.ld, nx)
    elif op == "pair_dots":
        rc = L.hipk_pair_dots(side.ctx, dt, m, xp, X.ld, yp, Y.ld, nx, dp)
    elif op == "scale":
        rc = L.hipk_scale_cols(side.ctx, dt, m, yp, Y.ld, nx, _dp(r))
    elif op == "rsqrt":
        rc = L.hipk_scale_cols_rsqrt_dev(side.ctx, dt, m, yp, Y.ld, nx, dp)
    elif op == "norms2":
        rc = L.hipk_col_norms2(side.ctx, dt, m, yp, Y.ld, nx, dp)
    elif op == "residual":
        rc = L.hipk_residual_cols(side.ctx, dt, m, xp, X.ld, yp, Y.ld, nx, _dp(r), dp)
    else:
        rc = L.hipk_gather_cols(side.ctx, dt, m, xp, X.ld, (C.c_int * nx)(*perm), nx, yp, Y.ld)
    assert rc == 0, f"{cid}: rc = {rc}"
    got = _check_guards(side, rep, cid, [("X", X), ("Y", Y), ("out", dres)], tens)
    gy, gd = Y.take(got[id(Y)], range(nx)), dres.take(got[id(dres)], 0)[0]
    if op == "axpy":          # y = a x + y, complex a
        zcmp(rep, f"{cid} Y", gy, al * xl + yl, sprod(al, absz(xl)) + absz(yl), lambda s: zbound_elem(dt, 1, s))
    elif op == "xpay":        # y = a y + x
        zcmp(rep, f"{cid} Y", gy, al * yl + xl, sprod(al, absz(yl)) + absz(xl), lambda s: zbound_elem(dt, 1, s))
    elif op == "pair_dots":   # out[c] = x_c^H y_c
        zcmp(rep, f"{cid} out", gd, (xl.conj() * yl).sum(1), sprod(xl, absz(yl)).sum(1), lambda s: zbound_red(m, s))
    elif op == "scale":       # real factors
        zcmp(rep, f"{cid} Y", gy, rl * yl, np.abs(rl) * absz(yl), lambda s: zbound_elem(dt, 1, s))
    elif op == "rsqrt":
        f = 1 / np.sqrt(np.asarray(np.linspace(0.3, 4.0, nx), LD))[:, None]
        zcmp(rep, f"{cid} Y", gy, f * yl, f * absz(yl), lambda s: zbound_elem(dt, 2, s))
    elif op == "norms2":
        rep.cmp(f"{cid} out", gd, n2z(yl), zbound_red(m, n2z(yl)))
    elif op == "residual":    # w -= theta x (theta real), |w|^2 as stored
        w, S = yl - rl * xl, absz(yl) + np.abs(rl) * absz(xl)
        zcmp(rep, f"{cid} W", gy, w, S, lambda s: zbound_elem(dt, 1, s))
        rep.cmp(f"{cid} nrm2", gd, n2z(_rz(w, dt)), zbound_red(m, n2z(S), dt, 1))
    else:
        rep.same_bits(f"{cid} Y(:,i) = X(:,perm[i])", gy, Xd[perm])


def _run_copy(side, c, rep):
    dt, m, nx = c["dt"], c["m"], c["nx"]
    cid, rng, npdt = case_id(c), _rng(c), np.dtype(NPDT[c["dt"]])
    Xd = _zrand(rng, (nx, m), dt) if npdt.kind == "c" else rng.standard_normal((nx, m)).astype(npdt)
    X, Y = Operand(npdt, m, nx, c["ldx"], c["shift"]), Operand(npdt, m, nx, c["ldy"], c["shift"])
    X.fill(range(nx), Xd); Y.expect(range(nx))
    tens = _upload(side, [X, Y])
    rc = side.lib.hipk_copy_cols(side.ctx, dt, m, X.base(side, tens[id(X)]), X.ld, Y.base(side, tens[id(Y)]), Y.ld, nx)
    assert rc == 0, f"{cid}: rc = {rc}"
    got = _check_guards(side, rep, cid, [("X", X), ("Y", Y)], tens)
    rep.same_bits(f"{cid} Y", Y.take(got[id(Y)], range(nx)), Xd)


RUNNERS = {"dots": _run_dots, "project": _run_project, "project_mul": _run_project_mul, "ritz_update": _run_ritz_update,
           "columns": _run_columns, "copy_cols": _run_copy}


def run_cases(side_factory, cases):
    return _run_cases(side_factory, cases, RUNNERS)


def groups(tables):
    """[(id, cases)]: the cases of the given tables by (table, type, flavour) — one test each"""
    out = {}
    for tb in tables:
        for c in CASES[tb]:
            out.setdefault("-".join(x for x in (tb, TNAME[c["dt"]], c.get("flavour", "")) if x), []).append(c)
    return sorted(out.items())
