"""Cases, operand layouts and high-precision references for the branch-by-branch tests of the real panel and Ritz
kernels (tests/test_panel_branches_host.py on the plain-C oracle, tests/test_panel_branches_gpu.py on the device).

Three parts:
  * layout(): every operand of a case sits inside one allocation [guard | operand | guard]; guards, the rows [m, ld) of
    every column, unused columns and spare output slots hold a quiet NaN.  An over-run therefore lands in memory the test
    owns, and it is seen either because the NaN reaches a sum or because the bit-for-bit comparison of everything the
    call must not write fails afterwards (integer views: NaN == NaN).
  * ref_*(): the operations in np.longdouble, written from the contract in include/primme_amd_kernels.h (NOT from the
    kernels and not from oracle/hipk_cpu.c), on exactly the inputs the device gets (already rounded to the panel type).
    Each returns, besides the result, the sum of absolute terms S its tolerance is proportional to.
  * the static case tables, branch_of() and cells_of(), and the runners behind run_cases() that drive one case on a
    kernel_harness side (Dev or Host) — the runners use ctypes only for the argument records.

Tolerances (derived, nothing tuned).  u64 = 2^-53, uT = unit round-off of the panel type, gamma(n, u) = n u / (1 - n u):
  * element-wise output of n products, rounded to T:                      2 gamma(n + 2, uT) S
  * reduction over m rows (double accumulation by contract) of inputs:    2 gamma(m + 2, u64) S
  * reduction whose operand is a computed vector r of n products/element: 2 (gamma(m + 2, u64) + gamma(n + 2, uT)) S
The factor 2 is for the reference's own longdouble error and fused against unfused products.  For a residual
r = W h - theta V h, n = 2 k (k products of each sum); each element of r is then off by at most gamma(k + 2, uT) S_r(i)
however it is accumulated, so that a product of TWO computed factors ((V h)' r, r' r) is off by 2 gamma(k + 2, uT)
<= 2 gamma(n + 2, uT) to first order: the same formula covers it.  S of such a reduction is sum_i |a_i| S_r(i) with
S_r(i) the absolute terms of r(i) (the error of r(i) is relative to S_r(i), not to |r(i)|).
"""
import ctypes as C
import zlib

import numpy as np

from primme_amd import _ffi as F

LD = np.longdouble
F64, F32 = F.HIPK_F64, F.HIPK_F32
NPDT = {F64: np.float64, F32: np.float32}
U64 = 2.0 ** -53
UNIT = {F64: 2.0 ** -53, F32: 2.0 ** -24}
GUARD = 64
TNAME = {F64: "f64", F32: "f32"}


def gamma(n, u):
    return n * u / (1.0 - n * u)


def bound_elem(dt, n, S):
    return 2.0 * gamma(n + 2, UNIT[dt]) * S


def bound_red(m, S, dt=None, n=None):
    g = gamma(m + 2, U64)
    if n is not None:
        g += gamma(n + 2, UNIT[dt])
    return 2.0 * g * S


# ------------------------------------------------------------------------------------------------------------------
# layouts
# ------------------------------------------------------------------------------------------------------------------
class Operand:
    """`rows` x `ncols` column-major block with leading dimension ld inside [GUARD | shift | ncols*ld | GUARD] elements,
    all NaN until fill() puts data in.  `written` marks what the call under test is expected to write; everything else
    must come back bit-identical."""

    def __init__(self, dtype, rows, ncols, ld, shift=0):
        self.dtype = np.dtype(dtype)
        self.rows, self.ncols, self.ld, self.shift = rows, ncols, max(int(ld), 1), shift
        self.off = GUARD + shift
        n = self.off + max(ncols, 1) * self.ld + GUARD
        self.host = np.full(n, np.nan, self.dtype)
        if self.dtype.kind == "c":
            self.host.imag = np.nan                  # a complex element is NaN in both halves
        self.written = np.zeros(n, bool)

    def index(self, cols, rows=None):
        cols = np.atleast_1d(np.asarray(cols, dtype=np.int64))
        r = np.arange(self.rows if rows is None else rows, dtype=np.int64)
        return self.off + cols[:, None] * self.ld + r[None, :]

    def fill(self, cols, data):
        self.host[self.index(cols)] = np.asarray(data, self.dtype).reshape(len(np.atleast_1d(cols)), self.rows)

    def expect(self, cols):
        self.written[self.index(cols)] = True

    def take(self, flat, cols):
        return flat[self.index(cols)]

    def base(self, side, t, col=0):
        return side.ptr(t, self.off + col * self.ld)


def layout(dt, m, ncols, flavour, extra=0):
    """One panel operand of type dt.  flavour:
      'vec'   every column 16-byte aligned: aligned base, ld = m rounded up to the vector width (ld == m, columns back
              to back, when m is a multiple of it; otherwise the shortest possible padding: every tail length occurs);
      'odd'   aligned base, odd ld (ld == m for odd m): switches the vector path off through the leading dimension;
      'shift' ld a multiple of the vector width, base moved by one element: switches it off through the base.
    extra widens ld without changing the flavour."""
    npdt = np.dtype(NPDT[dt])
    w = 16 // npdt.itemsize
    if flavour == "vec":
        return Operand(npdt, m, ncols, -(-m // w) * w + extra * w, 0)
    if flavour == "odd":
        return Operand(npdt, m, ncols, (m if m % 2 else m + 1) + 2 * extra, 0)
    assert flavour == "shift"
    return Operand(npdt, m, ncols, -(-m // w) * w + w + extra * w, 1)


def small(rows, ncols=1, spare=3):
    """array of doubles (coefficients, results): `rows` live entries per column, `spare` NaN slots behind them"""
    return Operand(np.float64, rows, ncols, rows + spare, 0)


def is_vec(dt, *ops):
    """aligned16 of csrc/hipk_panel_dev.h for every operand given (device allocations are 256-byte aligned)"""
    return all((op.off * op.dtype.itemsize) % 16 == 0 and (op.ld * op.dtype.itemsize) % 16 == 0 for op in ops)


# ------------------------------------------------------------------------------------------------------------------
# references (np.longdouble, from the header's contract).  Panels come as (ncols, m) arrays: row j = column j.
# ------------------------------------------------------------------------------------------------------------------
def _r(x, dt):
    """round to the panel type, back in longdouble"""
    return np.asarray(x, LD).astype(NPDT[dt]).astype(LD)


def ref_dots(A, X):
    """out[c, j] = col_j' X(:,c)"""
    A, X = np.asarray(A, LD), np.asarray(X, LD)
    return X @ A.T, np.abs(X) @ np.abs(A).T


def ref_project(dt, A, coef, X):
    """Xout(:,c) = X(:,c) - [segs] coef(:,c) with coef[c, j]; nrm2[c] = |Xout(:,c)|^2 of the stored columns"""
    A, X, coef = np.asarray(A, LD), np.asarray(X, LD), np.asarray(coef, LD)
    out = X - coef @ A
    S = np.abs(X) + np.abs(coef) @ np.abs(A)
    o = _r(out, dt)
    return out, S, (o * o).sum(axis=1), (S * S).sum(axis=1)


def ref_project_mul(A, coef, Mc, X):
    """X <- (X - [segs] coef) M with Mc[c, i] = M(i, c)"""
    A, X, coef, Mc = (np.asarray(a, LD) for a in (A, X, coef, Mc))
    Y = X - coef @ A
    SY = np.abs(X) + np.abs(coef) @ np.abs(A)
    return Mc @ Y, np.abs(Mc) @ SY


def ref_ritz_col(V, W, hc, theta, kind):
    """one job of hipk_ritz_update: (value, S) per row"""
    V, hc = np.asarray(V, LD), np.asarray(hc, LD)
    if kind == F.HIPK_JOB_XV:
        return hc @ V, np.abs(hc) @ np.abs(V)
    W = np.asarray(W, LD)
    if kind == F.HIPK_JOB_XW:
        return hc @ W, np.abs(hc) @ np.abs(W)
    th = LD(theta)
    return hc @ W - th * (hc @ V), np.abs(hc) @ np.abs(W) + abs(th) * (np.abs(hc) @ np.abs(V))


def ref_residual(dt, V, W, h, theta, Q, wtr):
    """dst = W h - theta V h; out = [V'dst | Q'dst | dst'dst (| W'dst | W(:,k-1)'Q)] with dst as stored.
    Returns r, S_r, out, S_out, computed (True where an operand of the reduction is the computed vector)."""
    r, Sr = ref_ritz_col(V, W, h, theta, F.HIPK_JOB_RES)
    V, W, Q = np.asarray(V, LD), np.asarray(W, LD), np.asarray(Q, LD)
    rt = _r(r, dt)
    out = [V @ rt, Q @ rt, [rt @ rt]]
    S = [np.abs(V) @ Sr, np.abs(Q) @ Sr, [Sr @ Sr]]
    comp = [np.ones(len(V), bool), np.ones(len(Q), bool), [True]]
    if wtr:
        out += [W @ rt, Q @ W[-1]]
        S += [np.abs(W) @ Sr, np.abs(Q) @ np.abs(W[-1])]
        comp += [np.ones(len(W), bool), np.zeros(len(Q), bool)]
    return r, Sr, np.concatenate(out), np.concatenate(S), np.concatenate(comp)


def ref_update_overlaps(dt, V, W, hv, hw, hr, theta_r, Q):
    """ov = [(V h)'r | Q'r | r'r | (W h)'r | W(:,k-1)'Q] for the nb new basis columns V hv[o], W hw[o] as stored"""
    r, Sr = ref_ritz_col(V, W, hr, theta_r, F.HIPK_JOB_RES)
    rt = _r(r, dt)
    V, W, Q, hv, hw = (np.asarray(a, LD) for a in (V, W, Q, hv, hw))
    xv, xw = _r(hv @ V, dt), _r(hw @ W, dt)
    Sv, Sw = np.abs(hv) @ np.abs(V), np.abs(hw) @ np.abs(W)
    out = np.concatenate([xv @ rt, Q @ rt, [rt @ rt], xw @ rt, Q @ W[-1]])
    S = np.concatenate([Sv @ Sr, np.abs(Q) @ Sr, [Sr @ Sr], Sw @ Sr, np.abs(Q) @ np.abs(W[-1])])
    comp = np.concatenate([np.ones(len(hv) + len(Q) + 1 + len(hw), bool), np.zeros(len(Q), bool)])
    return out, S, comp, (rt @ rt, Sr @ Sr)


def ref_project_triple(dt, A, coef, Wp, X, Vp):
    """W <- W - [segs] coef, out = [x'w | v'w | v'x] for the updated (stored) W"""
    w, Sw, _, _ = ref_project(dt, A, coef, Wp)
    wt = _r(w, dt)
    X, Vp = np.asarray(X, LD), np.asarray(Vp, LD)
    out = np.concatenate([(X * wt).sum(1), (Vp * wt).sum(1), (Vp * X).sum(1)])
    S = np.concatenate([(np.abs(X) * Sw).sum(1), (np.abs(Vp) * Sw).sum(1), (np.abs(Vp) * np.abs(X)).sum(1)])
    comp = np.concatenate([np.ones(2 * len(X), bool), np.zeros(len(X), bool)])
    return w, Sw, out, S, comp


# ------------------------------------------------------------------------------------------------------------------
# case tables (static: built by plain loops, nothing is chosen at run time)
# ------------------------------------------------------------------------------------------------------------------
M_SMALL = [1, 63, 65]                                            # below one step of every kernel family
M_LARGE = [64 * 2 * 5 + 77, 64 * 4 * 3 + 2, 1279, 716, 1463, 333, 1091, 514]   # several steps, tails of every length mod 4
M_LARGE_BIGK = [300, 269, 333]                                   # k up to 1023: 2.5 MB per panel
SCALAR_FLAVOURS = ["odd", "shift"]
TYPES = [F64, F32]


class _Rot:
    def __init__(self):
        self.i = 0

    def next(self, seq):
        self.i += 1
        return seq[(self.i - 1) % len(seq)]


def _flavour(vec, i):
    return "vec" if vec else SCALAR_FLAVOURS[i % 2]


def _residual_cases():
    out, rs, rl, n = [], _Rot(), _Rot(), 0
    kb = [(1, 8), (9, 16), (17, 24), (25, 32)]
    lb = [(0, 0), (1, 8), (9, 16), (17, 32)]
    for dt in TYPES:
        for vec in (True, False):
            for wtr in (0, 1):
                for (k0, k1) in kb:
                    for (l0, l1) in lb:
                        n += 1
                        out.append(dict(ep="residual", dt=dt, m=rs.next(M_SMALL), k=k0, L=l0, wtr=wtr, flavour=_flavour(vec, n), size="s"))
                        out.append(dict(ep="residual", dt=dt, m=rl.next(M_LARGE), k=k1, L=l1, wtr=wtr, flavour=_flavour(vec, n + 1), size="l"))
    return out


def _residual_dev_cases():
    out, n = [], 0
    for dt in TYPES:
        for vec in (True, False):
            for i, k in enumerate((5, 16, 17, 32)):
                n += 1
                out.append(dict(ep="residual_dev", dt=dt, m=[65, 717, 1279, 63][i], k=k, L=[0, 3, 9, 20][i], wtr=i % 2,
                                flavour=_flavour(vec, n), size="sl"[i % 2]))
    return out


PROJECT_NX = [1, 2, 3, 4, 5, 7, 8, 9, 15]
PROJECT_TOT = [1, 8, 192, 193]
PROJECT_SPLIT = [1, 2, 3]        # segments; 3 = three segments with the middle one empty


def _project_cases():
    out, rs, rl = [], _Rot(), _Rot()
    for dt in TYPES:
        for fi, flavour in enumerate(["vec", "odd", "shift"]):
            for ni, nx in enumerate(PROJECT_NX):
                for si, size in enumerate("sl"):
                    i = 2 * ni + si + fi
                    out.append(dict(ep="project", dt=dt, m=(rs if size == "s" else rl).next(M_SMALL if size == "s" else M_LARGE), nx=nx,
                                    tot=PROJECT_TOT[i % 4], split=PROJECT_SPLIT[(i // 2 + ni) % 3], norms=(i // 4 + si) % 2 == 0,
                                    place=["in", "out"][(ni + si + fi) % 2], flavour=flavour, fin=False, size=size))
            # the attributes the rotation above leaves uncovered for this (type, flavour), and the in-kernel second stage
            for ti, tot in enumerate(PROJECT_TOT):
                for split in PROJECT_SPLIT:
                    for norms in (True, False):
                        place = ["in", "out"][(ti + split + norms) % 2]
                        out.append(dict(ep="project", dt=dt, m=rl.next(M_LARGE) if (ti + split) % 2 else rs.next(M_SMALL), nx=[3, 5, 2, 9][ti],
                                        tot=tot, split=split, norms=norms, place=place, flavour=flavour, fin=False, size="l" if (ti + split) % 2 else "s"))
            for norms in (True, False):
                for place in ("in", "out"):
                    out.append(dict(ep="project", dt=dt, m=rl.next(M_LARGE), nx=7, tot=8, split=2, norms=norms, place=place, flavour=flavour,
                                    fin=False, size="l"))
            if flavour != "shift":
                for ni, nx in enumerate((1, 2, 4, 8)):
                    out.append(dict(ep="project", dt=dt, m=[65, 717, 1279, 63][ni], nx=nx, tot=[8, 1, 192, 8][ni], split=1 + ni % 3, norms=True,
                                    place=["in", "out"][ni % 2], flavour=flavour, fin=True, size="slls"[ni]))
    return out


def _project_mul_cases():
    out, rs, rl, n = [], _Rot(), _Rot(), 0
    for dt in TYPES:
        for vec in (True, False):
            for nx in range(1, 9):
                for ti, tot in enumerate((0, 1, 24)):
                    n += 1
                    size = "sl"[(nx + ti) % 2]
                    out.append(dict(ep="project_mul", dt=dt, m=(rs if size == "s" else rl).next(M_SMALL if size == "s" else M_LARGE), nx=nx, tot=tot,
                                    split=1 + (n % 3), flavour=_flavour(vec, n), size=size))
    # every (type, alignment, NX) instantiation at both row counts: the rotation above gives nx = 1..8 both, this pins it
    return out


def _dots_cases():
    out, rs, rl, n = [], _Rot(), _Rot(), 0
    for dt in TYPES:
        groups = [(False, nx, [1, 8, 9, 20]) for nx in (1, 2, 3, 4, 5, 8, 9)] + [(True, nx, [1, 8, 9, 20]) for nx in (1, 2, 3)]
        for vec, nx, tots in groups:
            for si, size in enumerate("sl"):
                n += 1
                out.append(dict(ep="dots", dt=dt, m=(rs if size == "s" else rl).next(M_SMALL if size == "s" else M_LARGE), nx=nx, tot=tots[(n + si) % 4],
                                split=1 + n % 3, flavour=_flavour(vec, n), size=size, nomfma=False))
        for nx in (4, 5, 16, 17):
            for ti, tot in enumerate((1, 16, 17, 33, 48)):
                n += 1
                size = "sl"[(ti + nx) % 2]
                out.append(dict(ep="dots", dt=dt, m=(rs if size == "s" else rl).next(M_SMALL if size == "s" else M_LARGE), nx=nx, tot=tot,
                                split=1 + n % 3, flavour="vec", size=size, nomfma=False))
        # both row counts for both tile counts of the matrix-core kernel
        for tot, size in ((16, "s"), (16, "l"), (48, "s"), (48, "l"), (1, "l"), (17, "s")):
            n += 1
            out.append(dict(ep="dots", dt=dt, m=(rs if size == "s" else rl).next(M_SMALL if size == "s" else M_LARGE), nx=5, tot=tot, split=1 + n % 3,
                            flavour="vec", size=size, nomfma=False))
    return out


def _dots_wide_cases():
    """run in a child process with HIPK_NO_MFMA=1 (the knob is read once per process)"""
    out, rs, rl, n = [], _Rot(), _Rot(), 0
    for dt in TYPES:
        for nx in (4, 5, 8):
            for size in "sl":
                n += 1
                out.append(dict(ep="dots", dt=dt, m=(rs if size == "s" else rl).next(M_SMALL if size == "s" else M_LARGE), nx=nx, tot=[9, 33, 48, 32][n % 4],
                                split=1 + n % 3, flavour="vec", size=size, nomfma=True))
    return out


RITZ_K = [1, 8, 9, 16, 17, 24, 25, 32, 33, 48, 49, 64, 65, 255, 256, 511, 512, 1023]
RITZ_NH = 6


def _ritz_jobs(k, nres, nxv, nxw):
    """in-place XV / XW on the first columns, one XV into a spare column, nres residual jobs (every third without a
    destination, the others into spare columns of W; one with slot -1 when there are at least three)"""
    jobs = [(F.HIPK_JOB_XV, c % RITZ_NH, ("V", c), -1) for c in range(nxv)]
    jobs.append((F.HIPK_JOB_XV, (nxv + 1) % RITZ_NH, ("E", 0), -1))
    jobs += [(F.HIPK_JOB_XW, (c + 2) % RITZ_NH, ("W", c), -1) for c in range(nxw)]
    slot = 0
    for r in range(nres):
        dst = None if r % 3 == 1 else ("W", k + r)
        if nres >= 3 and r == 2:
            jobs.append((F.HIPK_JOB_RES, (r + 1) % RITZ_NH, dst, -1))
        else:
            jobs.append((F.HIPK_JOB_RES, (r + 1) % RITZ_NH, dst, slot))
            slot += 1
    return jobs


def _ritz_update_cases():
    out, rs, rl, rb, n = [], _Rot(), _Rot(), _Rot(), 0
    nres_few, nres_many = [1, 2, 3, 4], [5, 8, 13, 16]
    for dt in TYPES:
        for ki, k in enumerate(RITZ_K):
            for si, size in enumerate("sl"):
                for many in (False, True):
                    n += 1
                    if k > 64 and many != (si == (ki % 2)):
                        continue                 # the staged kernels have one accumulator width: one job count per row count
                    nres = (nres_many if many else nres_few)[(ki + si) % 4]
                    m = rs.next(M_SMALL) if size == "s" else (rb.next(M_LARGE_BIGK) if k > 64 else rl.next(M_LARGE))
                    out.append(dict(ep="ritz_update", dt=dt, m=m, k=k, jobs=_ritz_jobs(k, nres, min(k, 3), min(k, 2)), necols=1,
                                    flavour=["vec", "odd", "shift"][n % 3], size=size))
        # more than RITZ_MAXOUT outputs in one list with a small basis: the staged kernel at k = 20
        for size in "sl":
            jobs = [(F.HIPK_JOB_XV, o % RITZ_NH, ("E", o), -1) for o in range(81)] + [(F.HIPK_JOB_XW, 1, ("W", 0), -1), (F.HIPK_JOB_RES, 2, ("W", 20), 0)]
            out.append(dict(ep="ritz_update", dt=dt, m=65 if size == "s" else 333, k=20, jobs=jobs, necols=81, flavour="vec", size=size))
    return out


def _update_overlaps_cases():
    out, rs, rl, n = [], _Rot(), _Rot(), 0
    for dt in TYPES:
        for (k0, k1) in ((1, 16), (17, 32)):
            for (b0, b1) in ((1, 8), (9, 16)):
                for (l0, l1) in ((0, 0), (1, 8), (9, 16), (17, 32)):
                    n += 1
                    out.append(dict(ep="update_overlaps", dt=dt, m=rs.next(M_SMALL), k=k0, nb=b0, L=l0, inplace=n % 2 == 0,
                                    flavour=["vec", "odd", "shift"][n % 3], size="s"))
                    out.append(dict(ep="update_overlaps", dt=dt, m=rl.next(M_LARGE), k=k1, nb=b1, L=l1, inplace=n % 2 == 1,
                                    flavour=["vec", "odd", "shift"][(n + 1) % 3], size="l"))
    return out


def _triple_cases():
    out, rs, rl, n = [], _Rot(), _Rot(), 0
    for dt in TYPES:
        for vec in (True, False):
            for nx in (1, 2, 3, 4, 5, 8):
                for size in "sl":
                    n += 1
                    out.append(dict(ep="triple", dt=dt, m=(rs if size == "s" else rl).next(M_SMALL if size == "s" else M_LARGE), nx=nx,
                                    tot=[1, 8, 9, 24][n % 4], split=1 + n % 3, flavour=_flavour(vec, n), size=size))
    return out


CASES = {
    "residual": _residual_cases(), "residual_dev": _residual_dev_cases(), "project": _project_cases(),
    "project_mul": _project_mul_cases(), "dots": _dots_cases(), "dots_wide": _dots_wide_cases(),
    "ritz_update": _ritz_update_cases(), "update_overlaps": _update_overlaps_cases(), "triple": _triple_cases(),
}

# Cases the plain-C oracle cannot run, by name and with the reason (nothing is skipped silently):
ORACLE_CANNOT = {
    "project/fin": "hipk_set_inkernel_fin exists only in the device library; the oracle has one second stage "
                   "(the same shapes run on it without the switch)",
    "dots_wide": "HIPK_NO_MFMA selects between device kernels; the oracle has one loop (the same shapes run on it as plain dots cases)",
}


def case_id(c):
    keys = [k for k in ("m", "k", "L", "nb", "nx", "tot", "split", "wtr", "norms", "place", "inplace", "flavour", "fin") if k in c]
    s = ",".join(f"{k}={c[k]}" for k in keys)
    if "jobs" in c:
        s += f",njobs={len(c['jobs'])}"
    return f"{c['ep']}[{TNAME[c['dt']]},{s}]"


# ------------------------------------------------------------------------------------------------------------------
# which instantiation a case runs
# ------------------------------------------------------------------------------------------------------------------
def _case_vec(c):
    """16-byte path: decided by the layout flavour of the case (every panel operand of a case has the same flavour)"""
    return c["flavour"] == "vec"


def _bucket(v, edges):
    for e in edges:
        if v <= e:
            return e
    raise ValueError(v)


def _chunks(nx):
    seq = []
    while nx > 0:
        s = 8 if nx >= 8 else 4 if nx >= 4 else 2 if nx >= 2 else 1
        seq.append(s)
        nx -= s
    return tuple(seq)


def branch_of(c):
    """The template instantiation(s) the documented dispatch sends a case to.  THIS MIRRORS THE HOST DISPATCH of
    csrc/hipk_panels.hip (panel_dots_t, panel_project_v, panel_project_mul_v, hipk_project_triple_dots) and
    csrc/hipk_ritz.hip (ritz_cgs_t / ritz_cgs_k / ritz_cgs_q, ritz_update_t / ritz_dispatch, ritz_ov_t / ritz_ov_q) and
    the alignment rule aligned16 / segs_aligned16 of csrc/hipk_panel_dev.h: when the dispatch changes, this function and
    the tables above change with it."""
    ep, dt, t = c["ep"], c["dt"], TNAME[c["dt"]]
    vw_full = 16 // np.dtype(NPDT[dt]).itemsize
    vec = _case_vec(c)
    if ep in ("residual", "residual_dev"):
        cpw = {8: 2, 16: 4, 24: 6, 32: 8}[_bucket(c["k"], (8, 16, 24, 32))]
        qpw = 0 if c["L"] == 0 else {8: 2, 16: 4, 32: 8}[_bucket(c["L"], (8, 16, 32))]
        return ("ritz_cgs_kernel", t, cpw, qpw, 2 if vec else 1, bool(c["wtr"]))
    if ep == "project":
        return ("project_kernel", t, tuple(sorted(set(_chunks(c["nx"])))), vw_full if vec else 1)
    if ep == "project_mul":
        return ("project_mul_kernel", t, _bucket(c["nx"], (2, 4, 8)), vw_full if vec else 1)
    if ep == "dots":
        nx, tot = c["nx"], c["tot"]
        if nx >= 4 and vec and not c["nomfma"]:
            return ("dots_mfma_kernel", t, 1 if tot <= 16 else 2)
        if nx >= 4 and vec and tot > 8:
            return ("dots_wide_kernel", t, 4 if nx <= 4 else 8, vw_full)
        return ("dots_kernel", t, _bucket(min(nx, 8), (1, 2, 4, 8)), vw_full if vec else 1)
    if ep == "ritz_update":
        k = c["k"]
        nxv = sum(1 for j in c["jobs"] if j[0] == F.HIPK_JOB_XV)
        nxw = sum(1 for j in c["jobs"] if j[0] == F.HIPK_JOB_XW)
        nres = sum(1 for j in c["jobs"] if j[0] == F.HIPK_JOB_RES)
        if k <= 64 and nxv <= 80 and nxw <= 80:
            nk = _bucket(k, (8, 16, 24, 32, 48, 64))
            return ("ritz_kernel", t, nk, 4 if nres <= 4 else 16, nk <= 32)
        return ("ritz_big_kernel", t, 32 if k <= 255 else 16 if k <= 511 else 8, "k<=64" if k <= 64 else "k>64")
    if ep == "update_overlaps":
        return ("ritz_ov_kernel", t, 16 if c["k"] <= 16 else 32, 8 if c["nb"] <= 8 else 16, 0 if c["L"] == 0 else _bucket(c["L"], (8, 16, 32)))
    if ep == "triple":
        return ("project_triple_kernel", t, _bucket(c["nx"], (2, 4, 8)))        # one row per lane whatever the alignment
    raise ValueError(ep)


def cells_of(c):
    """the cells of the issue's branch sets a case covers"""
    ep, t, vec = c["ep"], TNAME[c["dt"]], _case_vec(c)
    b = branch_of(c)
    if ep == "project":
        cells = {("inst", t, nxc, b[3]) for nxc in b[2]}
        cells |= {("nx", t, vec, c["nx"]), ("tot", t, vec, c["tot"]), ("split", t, vec, c["split"]), ("norms", t, vec, c["norms"]),
                  ("place", t, vec, c["place"]), ("flavour", t, c["flavour"])}
        if c["fin"]:
            cells.add(("fin", t, vec, c["nx"]))
        return cells
    if ep == "project_mul":
        return {b, ("nx", t, vec, c["nx"], c["tot"])}
    if ep == "dots":
        cells = {b, ("nx", t, vec, c["nx"])}
        if b[0] == "dots_mfma_kernel" and c["nx"] in (4, 5, 16, 17):
            cells.add(("mfma", t, c["nx"], c["tot"]))
        return cells
    if ep == "ritz_update":
        return {b, ("k", t, c["k"])}
    if ep == "triple":
        return {b, ("nx", t, vec, c["nx"])}
    return {b}


def wanted_cells(table):
    """the whole branch set of a case table"""
    want = set()
    for t in ("f64", "f32"):
        vwf = 2 if t == "f64" else 4
        if table == "residual":
            want |= {("ritz_cgs_kernel", t, cpw, qpw, vw, wt) for cpw in (2, 4, 6, 8) for qpw in (0, 2, 4, 8) for vw in (1, 2) for wt in (False, True)}
        elif table == "residual_dev":
            want |= {("ritz_cgs_kernel", t, cpw, qpw, vw, wt) for (cpw, qpw, wt) in ((2, 0, False), (4, 2, True), (6, 4, False), (8, 8, True)) for vw in (1, 2)}
        elif table == "project":
            for vec in (True, False):
                want |= {("inst", t, nxc, vwf if vec else 1) for nxc in (1, 2, 4, 8)}
                want |= {("nx", t, vec, nx) for nx in PROJECT_NX} | {("tot", t, vec, tot) for tot in PROJECT_TOT}
                want |= {("split", t, vec, s) for s in PROJECT_SPLIT} | {("norms", t, vec, b) for b in (True, False)}
                want |= {("place", t, vec, p) for p in ("in", "out")} | {("fin", t, vec, nx) for nx in (1, 2, 4, 8)}
            want |= {("flavour", t, f) for f in ("vec", "odd", "shift")}
        elif table == "project_mul":
            for vec in (True, False):
                want |= {("project_mul_kernel", t, nxc, vwf if vec else 1) for nxc in (2, 4, 8)}
                want |= {("nx", t, vec, nx, tot) for nx in range(1, 9) for tot in (0, 1, 24)}
        elif table == "dots":
            want |= {("dots_kernel", t, nxc, 1) for nxc in (1, 2, 4, 8)} | {("dots_kernel", t, nxc, vwf) for nxc in (1, 2, 4)}
            want |= {("dots_mfma_kernel", t, nt) for nt in (1, 2)}
            want |= {("nx", t, False, nx) for nx in (1, 2, 3, 4, 5, 8, 9)} | {("nx", t, True, nx) for nx in (1, 2, 3, 4, 5, 16, 17)}
            want |= {("mfma", t, nx, tot) for nx in (4, 5, 16, 17) for tot in (1, 16, 17, 33, 48)}
        elif table == "dots_wide":
            want |= {("dots_wide_kernel", t, nxc, vwf) for nxc in (4, 8)} | {("nx", t, True, nx) for nx in (4, 5, 8)}
        elif table == "ritz_update":
            want |= {("ritz_kernel", t, nk, nr, nk <= 32) for nk in (8, 16, 24, 32, 48, 64) for nr in (4, 16)}
            want |= {("ritz_big_kernel", t, r, "k>64") for r in (32, 16, 8)} | {("ritz_big_kernel", t, 32, "k<=64")}
            want |= {("k", t, k) for k in RITZ_K + [20]}
        elif table == "update_overlaps":
            want |= {("ritz_ov_kernel", t, nk, nb, qm) for nk in (16, 32) for nb in (8, 16) for qm in (0, 8, 16, 32)}
        elif table == "triple":
            want |= {("project_triple_kernel", t, nxc) for nxc in (2, 4, 8)}
            want |= {("nx", t, vec, nx) for vec in (True, False) for nx in (1, 2, 3, 4, 5, 8)}
    return want


def coverage(table):
    """(cells covered, cells wanted, instantiations that lack one of the two row counts)"""
    have, sizes = set(), {}
    for c in CASES[table]:
        have |= cells_of(c)
        for b in ({("inst",) + x[1:] for x in cells_of(c) if x[0] == "inst"} if c["ep"] == "project" else {branch_of(c)}):
            sizes.setdefault(b, set()).add(c["size"])
    one_size = sorted(str(b) for b, s in sizes.items() if s != {"s", "l"})
    if table == "residual_dev":
        one_size = []            # one case per (k bucket, alignment, type): the by-value table has both row counts of these kernels
    return have, wanted_cells(table), one_size


# ------------------------------------------------------------------------------------------------------------------
# runners: one case on one side (kernel_harness.Dev or Host)
# ------------------------------------------------------------------------------------------------------------------
def _bits(a):
    """one row of integers per element (two for a complex element: either half differing counts)"""
    a = np.ascontiguousarray(a).reshape(-1)
    parts = 2 if a.dtype.kind == "c" else 1
    return a.view(np.uint64 if a.dtype.itemsize // parts == 8 else np.uint32).reshape(a.size, parts)


class Report:
    """worst error-to-bound ratio and the list of failures of a group of cases"""

    def __init__(self):
        self.worst, self.fails, self.ncases = 0.0, [], 0

    def cmp(self, what, got, ref, bound):
        got, ref, bound = np.asarray(got, LD), np.asarray(ref, LD), np.asarray(bound, LD)
        if got.size == 0:
            return
        err = np.abs(got - ref)
        with np.errstate(divide="ignore", invalid="ignore"):
            ratio = np.where(bound > 0, err / np.where(bound > 0, bound, 1), np.where(err == 0, 0.0, np.inf))
        ratio = np.where(np.isfinite(got), ratio, np.inf)
        w = float(ratio.max())
        self.worst = max(self.worst, w)
        if not w <= 1.0:
            self.fails.append(f"{what}: error/bound = {w:.3g} at flat index {int(np.argmax(ratio))}")

    def same_bits(self, what, a, b):
        bad = np.flatnonzero((_bits(a) != _bits(b)).any(axis=1))
        if bad.size:
            self.fails.append(f"{what}: {bad.size} elements differ bit-wise, first at {int(bad[0])}")

    def guard(self, what, op, after):
        bad = np.flatnonzero((_bits(op.host) != _bits(after)).any(axis=1) & ~op.written)
        if bad.size:
            e = int(bad[0]) - op.off
            self.fails.append(f"{what}: {bad.size} guard/padding/input elements changed, first at column {e // op.ld} row {e % op.ld} "
                              f"(allocation index {int(bad[0])}, operand starts at {op.off}, ld {op.ld}, rows {op.rows})")

    def summary(self):
        return f"{self.ncases} cases, worst error/bound {self.worst:.3g}"


def _rng(c):
    return np.random.default_rng(zlib.crc32(case_id(c).encode()))


def _split(tot, kind):
    if kind == 1:
        return [tot]
    if kind == 2:
        return [tot - tot // 2, tot // 2]
    return [tot - tot // 2, 0, tot // 2]


def _make_segs(c, rng, dt, m, tot, split):
    """the basis columns over 1..3 segment operands (an empty segment still has a valid base)"""
    ops, A = [], rng.standard_normal((tot, m)).astype(NPDT[dt])
    j = 0
    for s, n in enumerate(_split(tot, split)):
        op = layout(dt, m, max(n, 1), c["flavour"], extra=s % 2)
        if n:
            op.fill(range(n), A[j:j + n])
        ops.append((op, n))
        j += n
    return ops, A


def _seg_array(side, ops, ts):
    arr = (F.HipkSeg * max(len(ops), 1))()
    for i, ((op, n), t) in enumerate(zip(ops, ts)):
        arr[i].base, arr[i].ld, arr[i].ncols = op.base(side, t).value, op.ld, n
    return arr


def _jobs_array(side, jobs, where):
    arr = (F.HipkJob * len(jobs))()
    for i, (kind, col, dst, slot) in enumerate(jobs):
        arr[i].kind, arr[i].col, arr[i].slot = kind, col, slot
        arr[i].dst = None if dst is None else where[dst[0]][0].base(side, where[dst[0]][1], dst[1]).value
    return arr


def _finish(side, rep, cid, pairs):
    """read everything back; guards of every operand; returns the flat arrays"""
    got = []
    for name, op, t in pairs:
        a = side.get(t)
        rep.guard(f"{cid} {name}", op, a)
        got.append(a)
    return got


def _run_residual(side, c, rep, dev_form=False):
    dt, m, k, L, wtr = c["dt"], c["m"], c["k"], c["L"], c["wtr"]
    cid, rng, npdt = case_id(c), _rng(c), NPDT[c["dt"]]
    Vd, Wd = rng.standard_normal((k, m)).astype(npdt), rng.standard_normal((k, m)).astype(npdt)
    Qd = rng.standard_normal((L, m)).astype(npdt)
    h, theta = rng.standard_normal(k) / np.sqrt(k), 0.37 + 0.01 * k
    nout = k + L + 1 + (k + L if wtr else 0)
    r, Sr, oref, So, comp = ref_residual(dt, Vd, Wd, h, theta, Qd, wtr)
    results = []
    for form in (("value", "dev") if dev_form else ("value",)):
        V, W, Q, out = layout(dt, m, k + 1, c["flavour"]), layout(dt, m, k, c["flavour"]), layout(dt, m, max(L, 1), c["flavour"], extra=1), small(nout)
        V.fill(range(k), Vd); W.fill(range(k), Wd)
        if L:
            Q.fill(range(L), Qd)
        V.expect(k); out.expect(0)
        hth = small(34, spare=2)
        hth.host[hth.off:hth.off + k] = h
        hth.host[hth.off + 32], hth.host[hth.off + 33] = theta, 0.0
        tv, tw, tq, to, th = (side.arr(o.host) for o in (V, W, Q, out, hth))
        if form == "value":
            hh = np.ascontiguousarray(h)
            rc = side.lib.hipk_ritz_residual_overlaps(side.ctx, dt, m, V.base(side, tv), W.base(side, tw), V.ld, k, hh.ctypes.data_as(C.c_void_p),
                                                      C.c_double(theta), V.base(side, tv, k), Q.base(side, tq), Q.ld, L, wtr, out.base(side, to))
        else:
            rc = side.lib.hipk_ritz_residual_overlaps_dev(side.ctx, dt, m, V.base(side, tv), W.base(side, tw), V.ld, k, hth.base(side, th),
                                                          V.base(side, tv, k), Q.base(side, tq), Q.ld, L, wtr, out.base(side, to))
        assert rc == 0, f"{cid} ({form}): rc = {rc}"
        gv, gw, gq, go, gh = _finish(side, rep, f"{cid} ({form})", [("V", V, tv), ("W", W, tw), ("Q", Q, tq), ("out", out, to), ("hth", hth, th)])
        dst, res = V.take(gv, k)[0], out.take(go, 0)[0]
        rep.cmp(f"{cid} ({form}) dst", dst, r, bound_elem(dt, 2 * k, Sr))
        rep.cmp(f"{cid} ({form}) out", res, oref, np.where(comp, bound_red(m, So, dt, 2 * k), bound_red(m, So)))
        results.append((dst, res))
    if dev_form:
        rep.same_bits(f"{cid} dst: coefficients from device memory against by value", results[0][0], results[1][0])
        rep.same_bits(f"{cid} out: coefficients from device memory against by value", results[0][1], results[1][1])


def _run_project(side, c, rep):
    dt, m, nx, tot = c["dt"], c["m"], c["nx"], c["tot"]
    cid, rng, npdt = case_id(c), _rng(c), NPDT[c["dt"]]
    segs, A = _make_segs(c, rng, dt, m, tot, c["split"])
    Xd = rng.standard_normal((nx, m)).astype(npdt)
    cf = rng.standard_normal((nx, tot)) / np.sqrt(tot)
    X = layout(dt, m, nx, c["flavour"])
    X.fill(range(nx), Xd)
    O = X if c["place"] == "in" else layout(dt, m, nx, c["flavour"], extra=1)
    O.expect(range(nx))
    coef, n2 = small(tot, nx), small(nx)
    coef.fill(range(nx), cf)
    if c["norms"]:
        n2.expect(0)
    ts = [side.arr(op.host) for op, _ in segs]
    tx, tc, tn = side.arr(X.host), side.arr(coef.host), side.arr(n2.host)
    to = tx if O is X else side.arr(O.host)
    sa = _seg_array(side, segs, ts)
    nptr = n2.base(side, tn) if c["norms"] else None
    old = side.lib.hipk_set_inkernel_fin(2) if c["fin"] else None
    try:
        if c["place"] == "in":
            rc = side.lib.hipk_panel_project(side.ctx, dt, m, sa, len(segs), coef.base(side, tc), coef.ld, X.base(side, tx), X.ld, nx, nptr)
        else:
            rc = side.lib.hipk_panel_project_to(side.ctx, dt, m, sa, len(segs), coef.base(side, tc), coef.ld, X.base(side, tx), X.ld,
                                                O.base(side, to), O.ld, nx, nptr)
        assert rc == 0, f"{cid}: rc = {rc}"
        pairs = [(f"seg{i}", op, t) for i, ((op, _), t) in enumerate(zip(segs, ts))] + [("X", X, tx), ("coef", coef, tc), ("nrm2", n2, tn)]
        if O is not X:
            pairs.append(("Xout", O, to))
        got = _finish(side, rep, cid, pairs)
    finally:
        if c["fin"]:
            side.lib.hipk_set_inkernel_fin(old)
    ref, S, nref, Sn = ref_project(dt, A, cf, Xd)
    rep.cmp(f"{cid} Xout", O.take(got[-1] if O is not X else got[len(segs)], range(nx)), ref, bound_elem(dt, tot, S))
    if c["norms"]:
        rep.cmp(f"{cid} nrm2", n2.take(got[len(segs) + 2], 0)[0], nref, bound_red(m, Sn, dt, tot))


def _run_project_mul(side, c, rep):
    dt, m, nx, tot = c["dt"], c["m"], c["nx"], c["tot"]
    cid, rng, npdt = case_id(c), _rng(c), NPDT[c["dt"]]
    segs, A = _make_segs(c, rng, dt, m, tot, c["split"])
    Xd = rng.standard_normal((nx, m)).astype(npdt)
    cf = rng.standard_normal((nx, tot)) / np.sqrt(max(tot, 1))
    Mc = rng.standard_normal((nx, nx)) / np.sqrt(nx)
    X, coef, Mo = layout(dt, m, nx, c["flavour"]), small(max(tot, 1), nx), Operand(np.float64, nx, nx, nx)
    X.fill(range(nx), Xd); X.expect(range(nx))
    if tot:
        coef.host[coef.index(range(nx), tot)] = cf
    Mo.fill(range(nx), Mc)
    ts = [side.arr(op.host) for op, _ in segs]
    tx, tc, tm = side.arr(X.host), side.arr(coef.host), side.arr(Mo.host)
    rc = side.lib.hipk_panel_project_mul(side.ctx, dt, m, _seg_array(side, segs, ts), len(segs), coef.base(side, tc), coef.ld, Mo.base(side, tm),
                                         X.base(side, tx), X.ld, nx)
    assert rc == 0, f"{cid}: rc = {rc}"
    got = _finish(side, rep, cid, [(f"seg{i}", op, t) for i, ((op, _), t) in enumerate(zip(segs, ts))] + [("coef", coef, tc), ("M", Mo, tm), ("X", X, tx)])
    ref, S = ref_project_mul(A, cf, Mc, Xd)
    rep.cmp(f"{cid} X", X.take(got[-1], range(nx)), ref, bound_elem(dt, nx * (tot + 1), S))


def _run_dots(side, c, rep):
    dt, m, nx, tot = c["dt"], c["m"], c["nx"], c["tot"]
    cid, rng, npdt = case_id(c), _rng(c), NPDT[c["dt"]]
    segs, A = _make_segs(c, rng, dt, m, tot, c["split"])
    A *= np.linspace(0.5, 2.0, tot)[:, None].astype(npdt)            # asymmetric: a row <-> column swap does not cancel
    j = 0
    for op, n in segs:
        if n:
            op.fill(range(n), A[j:j + n])
        j += n
    Xd = (rng.standard_normal((nx, m)) * np.linspace(1.0, 3.0, nx)[:, None]).astype(npdt)
    X, out = layout(dt, m, nx, c["flavour"], extra=1), small(tot, nx)
    X.fill(range(nx), Xd); out.expect(range(nx))
    ts = [side.arr(op.host) for op, _ in segs]
    tx, to = side.arr(X.host), side.arr(out.host)
    rc = side.lib.hipk_panel_dots(side.ctx, dt, m, _seg_array(side, segs, ts), len(segs), X.base(side, tx), X.ld, nx, out.base(side, to), out.ld)
    assert rc == 0, f"{cid}: rc = {rc}"
    got = _finish(side, rep, cid, [(f"seg{i}", op, t) for i, ((op, _), t) in enumerate(zip(segs, ts))] + [("X", X, tx), ("out", out, to)])
    ref, S = ref_dots(A, Xd)
    rep.cmp(f"{cid} out", out.take(got[-1], range(nx)), ref, bound_red(m, S))


def _run_ritz_update(side, c, rep):
    dt, m, k, jobs = c["dt"], c["m"], c["k"], c["jobs"]
    cid, rng, npdt = case_id(c), _rng(c), NPDT[c["dt"]]
    Vd, Wd = rng.standard_normal((k, m)).astype(npdt), rng.standard_normal((k, m)).astype(npdt)
    hc = rng.standard_normal((RITZ_NH, k)) / np.sqrt(k)
    theta = rng.standard_normal(RITZ_NH)
    nwx = max([d[1] + 1 for (_, _, d, _) in jobs if d and d[0] == "W"] + [k])
    nslots = max([s for (_, _, _, s) in jobs] + [-1]) + 1
    V, W, E = layout(dt, m, k, c["flavour"]), layout(dt, m, nwx, c["flavour"]), layout(dt, m, c["necols"], c["flavour"], extra=1)
    V.fill(range(k), Vd); W.fill(range(k), Wd)
    where_op = {"V": V, "W": W, "E": E}
    for (_, _, d, _) in jobs:
        if d:
            where_op[d[0]].expect(d[1])
    H, TH, N2 = small(k, RITZ_NH, spare=1), small(RITZ_NH), small(max(nslots, 1))
    H.fill(range(RITZ_NH), hc); TH.fill(0, theta)
    if nslots:
        N2.written[N2.index(0, nslots)] = True
    tv, tw, te, thh, tth, tn = (side.arr(o.host) for o in (V, W, E, H, TH, N2))
    arr = _jobs_array(side, jobs, {"V": (V, tv), "W": (W, tw), "E": (E, te)})
    rc = side.lib.hipk_ritz_update(side.ctx, dt, m, V.base(side, tv), W.base(side, tw), V.ld, k, H.base(side, thh), H.ld, TH.base(side, tth),
                                   arr, len(jobs), N2.base(side, tn))
    assert rc == 0, f"{cid}: rc = {rc}"
    gv, gw, ge, _, _, gn = _finish(side, rep, cid, [("V", V, tv), ("W", W, tw), ("E", E, te), ("h", H, thh), ("theta", TH, tth), ("nrm2", N2, tn)])
    flat = {"V": gv, "W": gw, "E": ge}
    for q, (kind, col, d, slot) in enumerate(jobs):
        ref, S = ref_ritz_col(Vd, Wd, hc[col], theta[col], kind)       # from the ORIGINAL panels: reads of a row precede its writes
        n = 2 * k if kind == F.HIPK_JOB_RES else k
        if d:
            rep.cmp(f"{cid} job {q} -> {d[0]}[{d[1]}]", where_op[d[0]].take(flat[d[0]], d[1])[0], ref, bound_elem(dt, n, S))
        if kind == F.HIPK_JOB_RES and slot >= 0:
            rt = _r(ref, dt)
            rep.cmp(f"{cid} job {q} nrm2[{slot}]", gn[N2.off + slot], rt @ rt, bound_red(m, S @ S, dt, n))


def _run_update_overlaps(side, c, rep):
    dt, m, k, nb, L, inplace = c["dt"], c["m"], c["k"], c["nb"], c["L"], c["inplace"]
    cid, rng, npdt = case_id(c), _rng(c), NPDT[c["dt"]]
    K0 = max(k, nb)
    ncol, off, nh, rescol = 2 * K0 + 2, (0 if inplace else K0), nb + 1, nb
    Vd, Wd = rng.standard_normal((k, m)).astype(npdt), rng.standard_normal((k, m)).astype(npdt)
    Qd = rng.standard_normal((L, m)).astype(npdt)
    hc = rng.standard_normal((nh, k)) / np.sqrt(k)
    theta = rng.standard_normal(nh)
    jobs = [(F.HIPK_JOB_XV, o, ("V", off + o), -1) for o in range(nb)] + [(F.HIPK_JOB_XV, rescol, ("V", 2 * K0 + 1), -1)]
    jobs += [(F.HIPK_JOB_XW, o, ("W", off + o), -1) for o in range(nb)] + [(F.HIPK_JOB_RES, rescol, ("W", 2 * K0), 0)]
    V, W, Q = layout(dt, m, ncol, c["flavour"]), layout(dt, m, ncol, c["flavour"]), layout(dt, m, max(L, 1), c["flavour"], extra=1)
    V.fill(range(k), Vd); W.fill(range(k), Wd)
    if L:
        Q.fill(range(L), Qd)
    for (_, _, d, _) in jobs:
        (V if d[0] == "V" else W).expect(d[1])
    nsl = 2 * nb + 2 * L + 1
    H, TH, N2, OV = small(k, nh, spare=2), small(nh), small(1), small(nsl)
    H.fill(range(nh), hc); TH.fill(0, theta); N2.expect(0); OV.expect(0)
    tv, tw, tq, thh, tth, tn, tov = (side.arr(o.host) for o in (V, W, Q, H, TH, N2, OV))
    arr = _jobs_array(side, jobs, {"V": (V, tv), "W": (W, tw)})
    rc = side.lib.hipk_ritz_update_overlaps(side.ctx, dt, m, V.base(side, tv), W.base(side, tw), V.ld, k, H.base(side, thh), H.ld, TH.base(side, tth),
                                            arr, len(jobs), N2.base(side, tn), nb, Q.base(side, tq), Q.ld, L, OV.base(side, tov))
    assert rc == 0, f"{cid}: rc = {rc}"
    gv, gw, _, _, _, gn, gov = _finish(side, rep, cid, [("V", V, tv), ("W", W, tw), ("Q", Q, tq), ("h", H, thh), ("theta", TH, tth),
                                                        ("nrm2", N2, tn), ("ov", OV, tov)])
    for q, (kind, col, d, slot) in enumerate(jobs):
        ref, S = ref_ritz_col(Vd, Wd, hc[col], theta[col], kind)
        op, flat = (V, gv) if d[0] == "V" else (W, gw)
        rep.cmp(f"{cid} job {q} -> {d[0]}[{d[1]}]", op.take(flat, d[1])[0], ref, bound_elem(dt, 2 * k if kind == F.HIPK_JOB_RES else k, S))
    oref, So, comp, (nref, Sn) = ref_update_overlaps(dt, Vd, Wd, hc[:nb], hc[:nb], hc[rescol], theta[rescol], Qd)
    rep.cmp(f"{cid} ov", OV.take(gov, 0)[0], oref, np.where(comp, bound_red(m, So, dt, 2 * k), bound_red(m, So)))
    rep.cmp(f"{cid} nrm2", gn[N2.off], nref, bound_red(m, Sn, dt, 2 * k))


def _run_triple(side, c, rep):
    dt, m, nx, tot = c["dt"], c["m"], c["nx"], c["tot"]
    cid, rng, npdt = case_id(c), _rng(c), NPDT[c["dt"]]
    segs, A = _make_segs(c, rng, dt, m, tot, c["split"])
    Wd, Xd, Vd = (rng.standard_normal((nx, m)).astype(npdt) for _ in range(3))
    cf = rng.standard_normal((nx, tot)) / np.sqrt(tot)
    Wp, X, Vp = layout(dt, m, nx, c["flavour"]), layout(dt, m, nx, c["flavour"], extra=1), layout(dt, m, nx, c["flavour"], extra=2)
    Wp.fill(range(nx), Wd); X.fill(range(nx), Xd); Vp.fill(range(nx), Vd); Wp.expect(range(nx))
    coef, out = small(tot, nx), small(3 * nx)
    coef.fill(range(nx), cf); out.expect(0)
    ts = [side.arr(op.host) for op, _ in segs]
    tw, tx, tv, tc, to = (side.arr(o.host) for o in (Wp, X, Vp, coef, out))
    rc = side.lib.hipk_project_triple_dots(side.ctx, dt, m, _seg_array(side, segs, ts), len(segs), coef.base(side, tc), coef.ld, Wp.base(side, tw), Wp.ld,
                                           nx, X.base(side, tx), X.ld, Vp.base(side, tv), Vp.ld, out.base(side, to))
    assert rc == 0, f"{cid}: rc = {rc}"
    got = _finish(side, rep, cid, [(f"seg{i}", op, t) for i, ((op, _), t) in enumerate(zip(segs, ts))] +
                  [("X", X, tx), ("V", Vp, tv), ("coef", coef, tc), ("W", Wp, tw), ("out", out, to)])
    w, Sw, oref, So, comp = ref_project_triple(dt, A, cf, Wd, Xd, Vd)
    rep.cmp(f"{cid} W", Wp.take(got[-2], range(nx)), w, bound_elem(dt, tot, Sw))
    rep.cmp(f"{cid} out", out.take(got[-1], 0)[0], oref, np.where(comp, bound_red(m, So, dt, tot), bound_red(m, So)))


_RUN = {"residual": _run_residual, "residual_dev": lambda s, c, r: _run_residual(s, c, r, dev_form=True), "project": _run_project,
        "project_mul": _run_project_mul, "dots": _run_dots, "ritz_update": _run_ritz_update, "update_overlaps": _run_update_overlaps,
        "triple": _run_triple}


def run_cases(side_factory, cases, runners=None):
    """all cases on ONE side object; returns the Report (the caller asserts on .fails and prints .summary()).
    runners: the table {entry point: runner} of another case module (tests/complex_branch_cases.py)"""
    rep = Report()
    side = side_factory()
    try:
        for c in cases:
            (runners or _RUN)[c["ep"]](side, c, rep)
            rep.ncases += 1
            if hasattr(side, "keep") and len(side.keep) > 64:
                _release(side)
    finally:
        _release(side)
        side.close()
    return rep


def _release(side):
    """give the buffers of the finished cases back (Dev frees device memory; Host drops its arrays)"""
    if side.name == "hip" and hasattr(side, "stage"):
        side.lib.hipk_sync(side.ctx)
        for t in side.keep:
            side.lib.hipk_free(side.ctx, C.c_void_p(t.ptr))
    side.keep = []


def groups(tables):
    """[(id, cases)]: the cases of the given tables by (entry point, type, alignment, flag) — one test each"""
    out = {}
    for tb in tables:
        for c in CASES[tb]:
            flag = f"wtr{c['wtr']}" if tb == "residual" else ("fin" if c.get("fin") else "")
            key = "-".join(x for x in (tb, TNAME[c["dt"]], "vec" if _case_vec(c) else "scalar", flag) if x)
            out.setdefault(key, []).append(c)
    return sorted(out.items())
