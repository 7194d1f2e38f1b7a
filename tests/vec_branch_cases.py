"""Cases, operand layouts and high-precision references for the branch-by-branch tests of csrc/hipk_vec.hip: the real column
utilities, the Jacobi preconditioner and the fused passes of the block-QMR inner solver (tests/test_vec_branches_host.py on the
plain-C oracle, tests/test_vec_branches_gpu.py on the device).  Operand, layout, the bounds and the Report idea come from
tests/panel_branch_cases.py.

  * Every operand of a case is an Operand [guard | operand | guard]; guards, the rows [m, ld) of every column, unused columns and
    spare result slots hold NaN (diag, tri / ggr and the result arrays included).  After the call everything the contract does not
    name as written must come back bit-identical (integer views).  No two panels of a case share a leading dimension.
  * ref_*(): np.longdouble, written from include/primme_amd_kernels.h (NOT from hipk_vec.hip or oracle/hipk_cpu.c), on the inputs
    already rounded to the panel type; a reference rounds to T where the header says a stored intermediate is rounded (the projected
    w, K^-1 g, the new delta and sol).  Each returns the sum of absolute terms S beside the value.
  * Bounds (nothing tuned; u64 = 2^-53, uT of the panel type, gamma(n, u) = n u / (1 - n u)):
        element of n rounded operations                 2 gamma(n + 2, uT) S
        reduction over m rows of inputs                 2 gamma(m + 2, u64) S
        reduction over computed elements                2 (gamma(m + 2, u64) + gamma(n + 2, uT)) S, S from the elements' own S
    A division counts as one operation and so does den = diag - shift (exact here, see below).  Operation counts:
        scale 1; 1/sqrt(norm2) scale 3; axpy / xpay 2; residual 2; delta = gamma delta + eta d 3; sol = delta + sol 4 (S = S_delta +
        |sol|); w = g / den 2; projected w 2; g -= alpha w_p 4; K^-1 g of that g 6; d = K^-1 g + beta d 4; gather / rotate 0 (exact).
  * The denominator guard: diag, the shifts and min_denominator are multiples of 2^-8 below 2^8, so that diag - shift is exact in
    float, double and longdouble and every precision takes the same clamp decision.  diag holds odd multiples and the shifts even
    ones (den is never zero by chance); the guard rows are then placed by hand, see guard_rows_of().
  * The `_dev` entry points are compared with the reference of their host-coefficient twins, with the coefficients formed in numpy
    float64, one rounding per operation, as the header writes them (qmr_coeffs()).
"""
import ctypes as C
import zlib

import numpy as np

from primme_amd import _ffi as F
from panel_branch_cases import GUARD, LD, Operand, Report, _bits, _release, bound_elem, bound_red, gamma, is_vec, layout, small

F64, F32, C64, C32 = F.HIPK_F64, F.HIPK_F32, F.HIPK_C64, F.HIPK_C32
RTYPES, ZTYPES = [F64, F32], [C64, C32]
REAL = {F64: F64, F32: F32, C64: F64, C32: F32}
NPDT = {F64: np.float64, F32: np.float32, C64: np.complex128, C32: np.complex64}
TNAME = {F64: "f64", F32: "f32", C64: "c64", C32: "c32"}
FLAVOURS = ["vec", "odd", "shift"]
MACH_EPS = 2.220446049250313e-16
MIND = 2.0 ** -4                    # min_denominator of the guard cases
STEP = 2.0 ** -8                    # diag, shifts, min_denominator are multiples of this
HIPK_BLOCK, ROWS_PER_WG, UTIL_MAXCOLS = 256, 1024, 64
NUM_CU = 256
"""compute units of the MI355X: the grid of every kernel here is min(ceil(m / rows per workgroup), NUM_CU * workgroups per CU);
branch_of / cells_of call a case "capped" from this constant (hipk_grid_for_rows reads the count from the device)"""
M_ROWS = [1, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 4099]
M_CAP = {4: ROWS_PER_WG * 4 * NUM_CU + 1029, 8: ROWS_PER_WG * 8 * NUM_CU + 1029}
M_WIDE = [65, 257, 255, 64, 256, 63, 1]          # rows of the cases that pin one column count (wide cases: m <= 257)

NX_UTIL = [1, 3, 64, 65, 129]
NX_ONE = [1, 3, 8, 64]
NX_CHUNK8 = [1, 7, 8, 9, 16, 17, 64]
NX_DEV = [1, 5, 8]
NX_JAC = [1, 3, 64]

# entry point -> (kernel, template flag or None, workgroups per CU of its grid, columns per launch or None, column counts, panels,
#                 written panels, result slots per column, has a denominator guard)
EPS = {
    "scale": ("scale_kernel", None, 8, 64, NX_UTIL, ("X",), ("X",), 0, False),
    "scale_rsqrt": ("scale_rsqrt_kernel", None, 8, None, NX_ONE, ("X",), ("X",), 0, False),
    "axpy": ("axpy_kernel", None, 8, 64, NX_UTIL, ("X", "Y"), ("Y",), 0, False),
    "xpay": ("xpay_kernel", None, 8, 64, NX_UTIL, ("X", "Y"), ("Y",), 0, False),
    "gather": ("gather_kernel", None, 8, 64, NX_UTIL, ("X", "Y"), ("Y",), 0, False),
    "norms2": ("norms2_kernel", None, 4, None, NX_ONE, ("X",), (), 1, False),
    "residual": ("residual_kernel", None, 4, 64, NX_UTIL, ("X", "W"), ("W",), 1, False),
    "rotate": ("pair_rotate_kernel", None, 8, None, NX_ONE, ("X", "Y"), ("Y",), 0, False),
    "pair_dots": ("pair_dots_kernel", None, 4, None, NX_ONE, ("X", "Y"), (), 1, False),
    "triple": ("triple_dots_kernel", None, 4, None, NX_ONE, ("X", "V", "W"), (), 3, False),
    "axpy_dot": ("axpy_dot_kernel", None, 4, None, NX_ONE, ("X", "Y", "Z"), ("Y",), 1, False),
    "axpy_dot_self": ("axpy_dot_kernel", None, 4, None, NX_ONE, ("X", "Y"), ("Y",), 1, False),
    "qmr_update": ("qmr_update_kernel", None, 4, None, NX_ONE, ("D", "Delta", "Sol"), ("Delta", "Sol"), 1, False),
    "qmr_update_jacobi": ("qmr_update_jacobi_kernel", None, 4, 8, NX_CHUNK8, ("D", "Delta", "Sol", "G", "W", "diag"), ("Delta", "Sol", "W"), 2, True),
    "axpy_proj_dot": ("axpy_proj_dot_kernel", None, 4, None, NX_ONE, ("W", "X", "G"), ("G",), 1, False),
    "axpy_proj_dot_jacobi": ("axpy_proj_dot_jacobi_kernel", False, 4, 8, NX_CHUNK8, ("W", "X", "G", "diag"), ("G",), 2, True),
    "axpy_proj_dot_jacobi_dev": ("axpy_proj_dot_jacobi_kernel", True, 4, None, NX_DEV, ("W", "X", "G", "diag"), ("G",), 2, True),
    "qmr_update_dir": ("qmr_update_dir_kernel", False, 4, 8, NX_CHUNK8, ("D", "Delta", "Sol", "G", "diag"), ("D", "Delta", "Sol"), 1, True),
    "qmr_update_dir_dev": ("qmr_update_dir_kernel", True, 4, None, NX_DEV, ("D", "Delta", "Sol", "G", "diag"), ("D", "Delta", "Sol"), 1, True),
    "jacobi": ("jacobi_kernel", None, 8, None, NX_JAC, ("x", "y", "diag"), ("y",), 0, True),
}
ENTRY = {"axpy_dot_self": "hipk_axpy_dot (Z == NULL)", "axpy_dot": "hipk_axpy_dot (Z)"}
OUTPUT_ONLY = {("gather", "Y"), ("rotate", "Y"), ("qmr_update_jacobi", "W"), ("jacobi", "y")}     # never read: stay NaN before the call
DEV_EPS = ("axpy_proj_dot_jacobi_dev", "qmr_update_dir_dev")
GUARD_ROWS = ("zero", "pos-small", "neg-small", "equal", "above")
GUARD_DEN = {"zero": 0.0, "pos-small": MIND / 2, "neg-small": -MIND / 2, "equal": -MIND, "above": MIND + STEP}


def is_z(dt):
    return dt in (C64, C32)


def _lay(dt, m, ncols, flavour, extra):
    """layout() of panel_branch_cases for the real types; the same three flavours for complex elements"""
    if not is_z(dt):
        return layout(dt, m, ncols, flavour, extra)
    npdt = np.dtype(NPDT[dt])
    w = max(16 // npdt.itemsize, 1)
    if flavour == "vec":
        return Operand(npdt, m, ncols, -(-m // w) * w + extra * w, 0)
    if flavour == "odd":
        return Operand(npdt, m, ncols, (m if m % 2 else m + 1) + 2 * extra, 0)
    return Operand(npdt, m, ncols, -(-m // w) * w + w + extra * w, 1)


# ------------------------------------------------------------------------------------------------------------------
# references (np.longdouble, from the header).  Panels are (ncols, m) arrays, coefficients (ncols,)
# ------------------------------------------------------------------------------------------------------------------
def _r(x, dt):
    return np.asarray(x, LD).astype(NPDT[REAL[dt]]).astype(LD)


def _col(v):
    return np.asarray(v, LD)[:, None]


def ref_scale(a, X):
    v = _col(a) * X
    return v, np.abs(v)


def ref_axpy(a, X, Y):
    """Y + a X"""
    return _col(a) * X + Y, np.abs(_col(a) * X) + np.abs(Y)


def ref_dot(A, B):
    return (A * B).sum(1), (np.abs(A) * np.abs(B)).sum(1)


def ref_den(diag, sh, mind):
    """diag - shift[c], |.| kept above min_denominator with its sign (min_denominator <= 0: 1e-300); a NaN stays"""
    md = LD(mind) if mind > 0 else LD(1e-300)
    den = np.asarray(diag, LD)[None, :] - _col(sh)
    with np.errstate(invalid="ignore"):
        return np.where(np.abs(den) <= md, np.copysign(md, den), den)


def ref_qmr(dt, gam, eta, D, De, So):
    """delta = gamma delta + eta d (stored), sol += delta (stored), |sol|^2"""
    nd = _col(gam) * De + _col(eta) * D
    Sd = np.abs(_col(gam) * De) + np.abs(_col(eta) * D)
    ns = _r(nd, dt) + So
    Ss = Sd + np.abs(So)
    return nd, Sd, ns, Ss, (_r(ns, dt) ** 2).sum(1), (Ss * Ss).sum(1)


def ref_proj(dt, al, xr, W, X, G):
    """g -= alpha (w - xr x) with the projected w rounded as if stored; |g|^2"""
    wp = W - _col(xr) * X
    Swp = np.abs(W) + np.abs(_col(xr) * X)
    g = G - _col(al) * _r(wp, dt)
    Sg = np.abs(G) + np.abs(_col(al)) * Swp
    return g, Sg, (_r(g, dt) ** 2).sum(1), (Sg * Sg).sum(1)


def qmr_alpha(tri, rho_prev, nx):
    """alpha and the dropped columns, numpy float64, one rounding per operation (header: sigma = 0 or not finite, |alpha| outside
    [eps, 1/eps])"""
    tri, rho_prev = np.asarray(tri, np.float64), np.asarray(rho_prev, np.float64)
    with np.errstate(all="ignore"):
        t = tri[:nx] * tri[2 * nx:3 * nx]
        sigma = tri[nx:2 * nx] - t
        alpha = rho_prev / sigma
        bad = ~np.isfinite(sigma) | (sigma == 0.0) | ~np.isfinite(alpha) | (np.abs(alpha) < MACH_EPS) | (np.abs(alpha) > 1.0 / MACH_EPS)
    return np.where(bad, 0.0, alpha), bad


def qmr_coeffs(ggr, alpha, rho_prev, tau_prev, theta_prev, nx):
    ggr = np.asarray(ggr, np.float64)
    with np.errstate(all="ignore"):
        theta = np.sqrt(ggr[:nx]) / tau_prev
        c = 1.0 / np.sqrt(1 + theta * theta)
        return ((c * c) * theta_prev) * theta_prev, (alpha * c) * c, ggr[nx:2 * nx] / rho_prev


# ------------------------------------------------------------------------------------------------------------------
# case tables (static)
# ------------------------------------------------------------------------------------------------------------------
def _shape_cases(ep, dt, k):
    kernel, flag, cap, chunk, nxs, *_ = EPS[ep]
    narrow = [n for n in nxs if n < 64]
    out = []
    for i, m in enumerate(M_ROWS):
        nx = nxs[(i + k) % len(nxs)]
        if nx >= 64 and m > 257:
            nx = narrow[(i + k) % len(narrow)]
        out.append(dict(ep=ep, dt=dt, m=m, nx=nx, flavour=FLAVOURS[(i + k) % 3]))
    for j, nx in enumerate(nxs):                         # every column count, at another row count and flavour than above
        out.append(dict(ep=ep, dt=dt, m=M_WIDE[(j + k) % len(M_WIDE)], nx=nx, flavour=FLAVOURS[(j + k + 1) % 3]))
    out.append(dict(ep=ep, dt=dt, m=M_CAP[cap], nx=2 if ep == "triple" else 1, flavour=FLAVOURS[k % 3], cap=True))
    if EPS[ep][8]:
        mid = nxs[len(nxs) // 2]
        out.append(dict(ep=ep, dt=dt, m=65, nx=mid, flavour=FLAVOURS[(k + 1) % 3], mind0=True))
        out.append(dict(ep=ep, dt=dt, m=257, nx=mid, flavour=FLAVOURS[(k + 2) % 3], noshift=True))
    if ep == "jacobi":
        out.append(dict(ep=ep, dt=dt, m=65, nx=3, flavour=FLAVOURS[k % 3], nanrow=True))
    return out


def _zjacobi_cases(dt, k):
    out = [dict(ep="jacobi", dt=dt, m=m, nx=NX_JAC[(i + k) % 3] if m <= 257 else [1, 3][i % 2], flavour=FLAVOURS[(i + k) % 3]) for i, m in enumerate(M_ROWS)]
    out += [dict(ep="jacobi", dt=dt, m=M_WIDE[j], nx=nx, flavour=FLAVOURS[(j + k + 1) % 3]) for j, nx in enumerate(NX_JAC)]
    out += [dict(ep="jacobi", dt=dt, m=M_CAP[8], nx=1, flavour=FLAVOURS[k % 3], cap=True),
            dict(ep="jacobi", dt=dt, m=65, nx=3, flavour=FLAVOURS[(k + 1) % 3], mind0=True),
            dict(ep="jacobi", dt=dt, m=257, nx=3, flavour=FLAVOURS[(k + 2) % 3], noshift=True),
            dict(ep="jacobi", dt=dt, m=65, nx=3, flavour=FLAVOURS[k % 3], nanrow=True)]
    return out


DROP_CLASSES = ("sigma0", "sigma_inf", "sigma_nan", "alpha_tiny", "rho0", "alpha_huge", "alpha_inf")
_RING = DROP_CLASSES + ("live",)


def _drop_cases():
    """columns that leave the block: every class in the first, a middle and the last column, a usable alpha beside them"""
    out, n = [], 0
    for dt in RTYPES:
        for nx in (1, 5, 8):
            for s in range(8):
                n += 1
                out.append(dict(ep="drop", dt=dt, m=[65, 257, 1025][n % 3], nx=nx, flavour=FLAVOURS[n % 3], classes=tuple(_RING[(c + s) % 8] for c in range(nx))))
        out.append(dict(ep="drop", dt=dt, m=65, nx=5, flavour="odd", classes=("sigma0", "alpha_tiny", "sigma_nan", "alpha_inf", "alpha_huge")))
    return out


RC_LIMIT64 = ("axpy_dot", "axpy_dot_self", "qmr_update", "qmr_update_jacobi", "axpy_proj_dot", "axpy_proj_dot_jacobi", "qmr_update_dir")
RC_REAL_ONLY = RC_LIMIT64 + ("triple", "axpy_proj_dot_jacobi_dev", "qmr_update_dir_dev", "rotate")


def _rc_cases():
    out, n = [], 0

    def add(ep, dt, nx, kind, rc):
        nonlocal n
        n += 1
        out.append(dict(ep=ep, dt=dt, m=37, nx=nx, flavour=FLAVOURS[n % 3], kind=kind, rc=rc))
    for dt in RTYPES:
        for ep in EPS:
            add(ep, dt, 3, "nx0", 0)
        for ep in RC_LIMIT64:
            add(ep, dt, 65, "nx65", -1)
        for ep in DEV_EPS:
            add(ep, dt, 9, "nx9", -1)
            add(ep, dt, 5, "tri_null", -1)
        add("qmr_update_dir_dev", dt, 5, "ggr_null", -1)
    for dt in RTYPES + ZTYPES:
        add("jacobi", dt, 65, "nx65", -1)
    for dt in ZTYPES:
        add("jacobi", dt, 3, "nx0", 0)
        for ep in RC_REAL_ONLY:
            add(ep, dt, 3, "complex", -44)
    return out


CASES = [c for k, ep in enumerate(EPS) for dt in RTYPES for c in _shape_cases(ep, dt, k)] + [c for k, dt in enumerate(ZTYPES) for c in _zjacobi_cases(dt, k)]
DROP = _drop_cases()
RC = _rc_cases()


def case_id(c):
    extra = "".join(f",{k}" for k in ("cap", "mind0", "noshift", "nanrow") if c.get(k))
    if "classes" in c:
        extra += "," + "/".join(c["classes"])
    if "kind" in c:
        extra += f",{c['kind']}"
    return f"{c['ep']}[{TNAME[c['dt']]},m={c['m']},nx={c['nx']},{c['flavour']}{extra}]"


def _rng(c):
    return np.random.default_rng(zlib.crc32(case_id(c).encode()))


def guard_rows_of(c):
    """[(row, column, class)]: where a case with a guard places den == 0, 0 < den < min_den, -min_den < den < 0, |den| == min_den and
    den just above min_den: against the LAST column's shift in the first rows and, when there is room, against the first column's
    shift in the last rows.  Not with min_denominator = 0 (every den stays non-zero there)."""
    m, nx = c["m"], c["nx"]
    if c["ep"] != "drop" and not EPS[c["ep"]][8] or c.get("mind0"):
        return []
    rot = (m + nx) % 5
    rows = [(r, nx - 1, GUARD_ROWS[(r + rot) % 5]) for r in range(min(5, m))]
    if m >= 10 and nx > 1:
        rows += [(m - 5 + r, 0, GUARD_ROWS[(r + rot) % 5]) for r in range(5)]
    return rows


# ------------------------------------------------------------------------------------------------------------------
# which launches a case makes
# ------------------------------------------------------------------------------------------------------------------
def kernel_of(c):
    if c["ep"] == "jacobi" and is_z(c["dt"]):
        return ("zjacobi_kernel", TNAME[c["dt"]])
    kernel, flag = EPS[c["ep"]][:2]
    return (kernel, TNAME[c["dt"]]) + (() if flag is None else (flag,))


def branch_of(c):
    """[(kernel, type[, DEV flag], c0)] for every launch of the call.  THIS MIRRORS THE HOST DISPATCH of csrc/hipk_vec.hip (and
    hipk_z_jacobi of csrc/hipk_complex.hip): the utilities launch once per UTIL_MAXCOLS = 64 columns, the three fused passes with the
    diagonal once per 8 columns (launch c0 writes its partial sums at which * nx + c0 + c), everything else once.  When the dispatch
    changes, this function and EPS change with it."""
    chunk = None if kernel_of(c)[0] == "zjacobi_kernel" else EPS[c["ep"]][3]
    return [kernel_of(c) + (c0,) for c0 in (range(0, c["nx"], chunk) if chunk else [0])]


def _rows_per_wg(c):
    return HIPK_BLOCK if kernel_of(c)[0] == "zjacobi_kernel" else ROWS_PER_WG


def cells_of(c):
    """(row cell, column cell).  Rows: one-lane (m = 1), waves (one trip), trips (one workgroup, several trips), blocks (several
    workgroups), capped (more rows than NUM_CU * workgroups per CU * rows per workgroup: the grid stride is taken).  Columns: 1,
    several, full-chunk (as many as one launch takes: 64, or 8 for the passes with the diagonal and the _dev forms), next-chunk."""
    m, nx, rpw = c["m"], c["nx"], _rows_per_wg(c)
    need = -(-m // rpw)
    row = ("one-lane" if m == 1 else "waves" if m <= HIPK_BLOCK else "trips" if need == 1 else
           "capped" if need > NUM_CU * EPS[c["ep"]][2] else "blocks")
    full = 8 if c["ep"] in DEV_EPS else (EPS[c["ep"]][3] or UTIL_MAXCOLS)
    if kernel_of(c)[0] == "zjacobi_kernel":
        full = UTIL_MAXCOLS
    col = "1" if nx == 1 else "several" if nx < full else "full-chunk" if nx == full else "next-chunk"
    return row, col


ROW_CELLS = ("one-lane", "waves", "trips", "blocks", "capped")
COL_CELLS = ("1", "several", "full-chunk", "next-chunk")
_ONE_LAUNCH = "one launch takes every column the entry point accepts"
NO_CELL = {k: {"next-chunk": _ONE_LAUNCH} for k in
           ("scale_rsqrt_kernel", "pair_rotate_kernel", "norms2_kernel", "pair_dots_kernel", "triple_dots_kernel", "axpy_dot_kernel",
            "qmr_update_kernel", "axpy_proj_dot_kernel", "jacobi_kernel", "zjacobi_kernel")}
NO_CELL["axpy_proj_dot_jacobi_kernel<DEV>"] = {"next-chunk": "the _dev form takes at most 8 columns: one launch"}
NO_CELL["qmr_update_dir_kernel<DEV>"] = {"next-chunk": "the _dev form takes at most 8 columns: one launch"}
NO_CELL["zjacobi_kernel"]["trips"] = "hipk_z_jacobi gives every 256 rows a workgroup: a lane makes a second trip only once the grid is capped"


def kernel_key(b):
    return b[0] + ("<DEV>" if len(b) > 2 and b[2] is True else "")


# ------------------------------------------------------------------------------------------------------------------
# operands of a case
# ------------------------------------------------------------------------------------------------------------------
def _panel_names(ep):
    return EPS[ep][5] if ep != "drop" else ("W", "X", "G", "D", "Delta", "Sol", "diag")


def panels(c):
    """the panel operands of a case, NaN everywhere: no two with the same leading dimension"""
    ep, dt, m, nx = c["ep"], c["dt"], c["m"], c["nx"]
    ops = {}
    for i, nm in enumerate(_panel_names(ep)):
        rows = 2 * m if ep == "rotate" else m
        ncols = 1 if nm == "diag" else nx + 1 if (ep, nm) == ("gather", "X") else nx
        ops[nm] = _lay(dt, rows, ncols, c["flavour"], i)
    return ops


def gather_perm(nx):
    """not the identity, and with a repeated source column when there is more than one"""
    p = [nx - i for i in range(nx)]
    if nx > 1:
        p[-1] = p[0]
    return p


def build(c):
    """(operands, host scalars, the raw (ncols, m) data) of a case; operands filled, `written` marked for the entry point's call"""
    ep, dt, m, nx = c["ep"], c["dt"], c["m"], c["nx"]
    rng, npdt = _rng(c), NPDT[dt]
    ops, d, s = panels(c), {}, {}
    for nm, op in ops.items():
        if nm == "diag" or (ep, nm) in OUTPUT_ONLY:
            continue
        d[nm] = rng.standard_normal((op.ncols, op.rows)).astype(npdt)
        if is_z(dt):
            d[nm] = (d[nm] + 1j * rng.standard_normal((op.ncols, op.rows))).astype(npdt)
        op.fill(range(op.ncols), d[nm])
    for k in ("a", "theta", "gam", "eta", "beta", "alpha", "xr"):
        s[k] = rng.standard_normal(nx) * 1.5
    s["n2"] = 0.5 + 4.0 * rng.random(nx)
    s["perm"] = gather_perm(nx)
    if "diag" in ops:
        s["mind"] = 0.0 if c.get("mind0") else MIND
        s["shift"] = None if c.get("noshift") else 2.0 * (rng.permutation(400)[:nx] - 200) * STEP
        diag = (2.0 * rng.integers(-1000, 1000, m) + 1.0) * STEP
        sh = np.zeros(nx) if s["shift"] is None else s["shift"]
        for row, col, cls in guard_rows_of(c):
            diag[row] = sh[col] + GUARD_DEN[cls]
        if c.get("nanrow"):
            diag[m // 2] = np.nan
        d["diag"] = diag.astype(npdt)[None, :]
        if is_z(dt):
            d["diag"] = (d["diag"].real + 1j * rng.standard_normal((1, m))).astype(npdt)       # only the real part counts
        ops["diag"].fill(0, d["diag"])
        s["shift0"] = sh
    s["tri"] = rng.standard_normal(3 * nx) * 3.0
    s["ggr"] = np.concatenate([0.5 + rng.random(nx) * 4.0, rng.standard_normal(nx) * 2.0])
    s["rho_prev"], s["tau_prev"], s["theta_prev"] = (np.abs(rng.standard_normal(nx)) + 0.1 for _ in range(3))
    nres = EPS[ep][7] if ep != "drop" else 2
    if nres:
        ops["out"] = small(nres * nx)
        ops["out"].expect(0)
    if ep == "scale_rsqrt":
        ops["n2"] = small(nx)
        ops["n2"].fill(0, s["n2"])
    if ep in DEV_EPS or ep == "drop":
        ops["tri"], ops["ggr"] = small(3 * nx), small(2 * nx)
        ops["tri"].fill(0, s["tri"])
        ops["ggr"].fill(0, s["ggr"])
    for nm in (EPS[ep][6] if ep != "drop" else ()):
        ops[nm].expect(range(nx))
    return ops, s, d


class Bed:
    """one upload of the operands of a case on a side"""

    def __init__(self, side, ops):
        self.side, self.ops = side, ops
        self.t = {k: side.arr(o.host) for k, o in ops.items()}

    def p(self, k, col=0):
        return self.ops[k].base(self.side, self.t[k], col) if k in self.ops else None

    def ld(self, k):
        return self.ops[k].ld if k in self.ops else 0

    def get(self):
        return {k: self.side.get(t) for k, t in self.t.items()}

    def fetch(self, rep, cid):
        got = self.get()
        for k, op in self.ops.items():
            rep.guard(f"{cid} {k}", op, got[k])
        return got


def _da(v):
    return None if v is None else (C.c_double * len(v))(*[float(x) for x in v])


def call(ep, side, b, s, m, nx, dt, col=0, n1=None):
    """the entry point of a case on the operands of bed b; col / n1: the n1 columns from `col` on (coefficients likewise)"""
    L, ctx, md = side.lib, side.ctx, C.c_double(s.get("mind", 0.0))
    n = nx if n1 is None else n1

    def a(k):
        return None if s.get(k) is None else _da(np.asarray(s[k])[col:col + max(n, 1)] if n1 is not None else s[k])

    def p(k):
        return b.p(k, col)
    if ep == "scale":
        return L.hipk_scale_cols(ctx, dt, m, p("X"), b.ld("X"), n, a("a"))
    if ep == "scale_rsqrt":
        return L.hipk_scale_cols_rsqrt_dev(ctx, dt, m, p("X"), b.ld("X"), n, b.p("n2"))
    if ep == "axpy":
        return L.hipk_axpy_cols(ctx, dt, m, a("a"), p("X"), b.ld("X"), p("Y"), b.ld("Y"), n)
    if ep == "xpay":
        return L.hipk_xpay_cols(ctx, dt, m, a("a"), p("X"), b.ld("X"), p("Y"), b.ld("Y"), n)
    if ep == "gather":
        return L.hipk_gather_cols(ctx, dt, m, p("X"), b.ld("X"), (C.c_int * max(n, 1))(*s["perm"][:max(n, 1)]), n, p("Y"), b.ld("Y"))
    if ep == "norms2":
        return L.hipk_col_norms2(ctx, dt, m, p("X"), b.ld("X"), n, b.p("out"))
    if ep == "residual":
        return L.hipk_residual_cols(ctx, dt, m, p("X"), b.ld("X"), p("W"), b.ld("W"), n, a("theta"), b.p("out"))
    if ep == "rotate":
        return L.hipk_pair_rotate(ctx, dt, m, p("X"), b.ld("X"), p("Y"), b.ld("Y"), n)
    if ep == "pair_dots":
        return L.hipk_pair_dots(ctx, dt, m, p("X"), b.ld("X"), p("Y"), b.ld("Y"), n, b.p("out"))
    if ep == "triple":
        return L.hipk_triple_dots(ctx, dt, m, p("X"), b.ld("X"), p("V"), b.ld("V"), p("W"), b.ld("W"), n, b.p("out"))
    if ep in ("axpy_dot", "axpy_dot_self"):
        return L.hipk_axpy_dot(ctx, dt, m, n, a("a"), p("X"), b.ld("X"), p("Y"), b.ld("Y"), p("Z") if ep == "axpy_dot" else None, b.ld("Z"), b.p("out"))
    if ep == "qmr_update":
        return L.hipk_qmr_update(ctx, dt, m, n, a("gam"), a("eta"), p("D"), b.ld("D"), p("Delta"), b.ld("Delta"), p("Sol"), b.ld("Sol"), b.p("out"))
    if ep == "qmr_update_jacobi":
        return L.hipk_qmr_update_jacobi(ctx, dt, m, n, a("gam"), a("eta"), p("D"), b.ld("D"), p("Delta"), b.ld("Delta"), p("Sol"), b.ld("Sol"),
                                        p("G"), b.ld("G"), b.p("diag"), a("shift"), md, p("W"), b.ld("W"), b.p("out"))
    if ep == "axpy_proj_dot":
        return L.hipk_axpy_proj_dot(ctx, dt, m, n, a("alpha"), a("xr"), p("W"), b.ld("W"), p("X"), b.ld("X"), p("G"), b.ld("G"), b.p("out"))
    if ep == "axpy_proj_dot_jacobi":
        return L.hipk_axpy_proj_dot_jacobi(ctx, dt, m, n, a("alpha"), a("xr"), p("W"), b.ld("W"), p("X"), b.ld("X"), p("G"), b.ld("G"),
                                           b.p("diag"), a("shift"), md, b.p("out"))
    if ep == "axpy_proj_dot_jacobi_dev":
        return L.hipk_axpy_proj_dot_jacobi_dev(ctx, dt, m, n, None if s.get("tri_null") else b.p("tri"), a("rho_prev"), C.c_double(MACH_EPS),
                                               p("W"), b.ld("W"), p("X"), b.ld("X"), p("G"), b.ld("G"), b.p("diag"), a("shift"), md, b.p("out"))
    if ep == "qmr_update_dir":
        return L.hipk_qmr_update_dir(ctx, dt, m, n, a("gam"), a("eta"), a("beta"), p("D"), b.ld("D"), p("Delta"), b.ld("Delta"), p("Sol"), b.ld("Sol"),
                                     p("G"), b.ld("G"), b.p("diag"), a("shift"), md, b.p("out"))
    if ep == "qmr_update_dir_dev":
        return L.hipk_qmr_update_dir_dev(ctx, dt, m, n, None if s.get("tri_null") else b.p("tri"), None if s.get("ggr_null") else b.p("ggr"),
                                         a("rho_prev"), a("tau_prev"), a("theta_prev"), C.c_double(MACH_EPS), p("D"), b.ld("D"),
                                         p("Delta"), b.ld("Delta"), p("Sol"), b.ld("Sol"), p("G"), b.ld("G"), b.p("diag"), a("shift"), md, b.p("out"))
    if ep == "jacobi":
        return jacobi(side, b, s, m, n, dt, "x", "y", col)
    raise ValueError(ep)


def jacobi(side, b, s, m, n, dt, src, dst, col=0, n1=None):
    sh = None if s.get("shift") is None else _da(np.asarray(s["shift"])[col:col + max(n, 1)])
    return side.lib.hipk_jacobi_apply(C.c_void_p(side.lib.hipk_ctx_stream(side.ctx)), dt, m, b.p("diag"), sh, C.c_double(s.get("mind", 0.0)),
                                      b.p(src, col), b.ld(src), b.p(dst, col), b.ld(dst), n)


# ------------------------------------------------------------------------------------------------------------------
# runners
# ------------------------------------------------------------------------------------------------------------------
class VReport(Report):
    """Report of panel_branch_cases with the worst ratio per layout flavour and the notes of the run beside it"""

    def __init__(self):
        super().__init__()
        self.by, self.notes, self.flavour = {}, [], None

    def cmp(self, what, got, ref, bound):
        before, self.worst = self.worst, 0.0
        super().cmp(what, got, ref, bound)
        self.by[self.flavour] = max(self.by.get(self.flavour, 0.0), self.worst)
        self.worst = max(before, self.worst)

    def summary(self):
        per = ", ".join(f"{k} {v:.3g}" for k, v in sorted(self.by.items()))
        return super().summary() + (f" ({per})" if per else "") + "".join(f"; {n}" for n in self.notes)


def _take(ops, got, k):
    return ops[k].take(got[k], range(ops[k].ncols))


def _same(rep, what, ops, names, got_a, got_b):
    for k in names:
        rep.same_bits(f"{what}: {k}", got_a[k], got_b[k])


def _scratch(c, like, data):
    op = _lay(c["dt"], like.rows, like.ncols, c["flavour"], 7)
    if data is not None:
        op.fill(range(like.ncols), data)
    return op


def _check_ref(rep, cid, c, ops, s, d, got):
    """the written panels and the result slots of the case against the longdouble reference"""
    ep, dt, m, nx = c["ep"], c["dt"], c["m"], c["nx"]
    rdt = REAL[dt]
    D = {k: np.asarray(v, np.clongdouble if is_z(dt) else LD) for k, v in d.items()}
    out = ops["out"].take(got["out"], 0)[0] if "out" in ops else None

    def el(k, ref, n, S):
        rep.cmp(f"{cid} {k}", _take(ops, got, k), ref, bound_elem(rdt, n, S))

    def red(slot, ref, S, n=None):
        rep.cmp(f"{cid} out[{slot} nx + c]", out[slot * nx:(slot + 1) * nx], ref, bound_red(m, S, rdt, n) if n else bound_red(m, S))
    if ep == "scale":
        v, S = ref_scale(s["a"], D["X"])
        el("X", v, 1, S)
    elif ep == "scale_rsqrt":
        v = D["X"] / np.sqrt(_col(s["n2"]))
        el("X", v, 3, np.abs(v))
    elif ep == "axpy":
        v, S = ref_axpy(s["a"], D["X"], D["Y"])
        el("Y", v, 2, S)
    elif ep == "xpay":
        v, S = ref_axpy(s["a"], D["Y"], D["X"])
        el("Y", v, 2, S)
    elif ep == "gather":
        el("Y", D["X"][s["perm"]], 0, 0.0 * np.abs(D["X"][s["perm"]]))
    elif ep == "rotate":
        v = np.empty_like(D["X"])
        v[:, 0::2], v[:, 1::2] = -D["X"][:, 1::2], D["X"][:, 0::2]
        el("Y", v, 0, 0.0 * np.abs(v))
    elif ep == "norms2":
        red(0, *ref_dot(D["X"], D["X"]))
    elif ep == "residual":
        v, S = ref_axpy(-np.asarray(s["theta"]), D["X"], D["W"])
        el("W", v, 2, S)
        red(0, (_r(v, dt) ** 2).sum(1), (S * S).sum(1), 2)
    elif ep == "pair_dots":
        red(0, *ref_dot(D["X"], D["Y"]))
    elif ep == "triple":
        red(0, *ref_dot(D["X"], D["W"]))
        red(1, *ref_dot(D["V"], D["W"]))
        red(2, *ref_dot(D["V"], D["X"]))
    elif ep in ("axpy_dot", "axpy_dot_self"):
        v, S = ref_axpy(s["a"], D["X"], D["Y"])
        el("Y", v, 2, S)
        if ep == "axpy_dot":
            red(0, (D["Z"] * _r(v, dt)).sum(1), (np.abs(D["Z"]) * S).sum(1), 2)
        else:
            red(0, (_r(v, dt) ** 2).sum(1), (S * S).sum(1), 2)
    elif ep in ("qmr_update", "qmr_update_jacobi", "qmr_update_dir", "qmr_update_dir_dev"):
        gam, eta, beta = s["gam"], s["eta"], s["beta"]
        if ep == "qmr_update_dir_dev":
            alpha, bad = qmr_alpha(s["tri"], s["rho_prev"], nx)
            assert not bad.any(), cid
            gam, eta, beta = qmr_coeffs(s["ggr"], alpha, s["rho_prev"], s["tau_prev"], s["theta_prev"], nx)
        nd, Sd, ns, Ss, o, So = ref_qmr(dt, gam, eta, D["D"], D["Delta"], D["Sol"])
        el("Delta", nd, 3, Sd)
        el("Sol", ns, 4, Ss)
        red(0, o, So, 4)
        if ep != "qmr_update":
            w = D["G"] / ref_den(D["diag"][0], s["shift0"], s["mind"])
            if ep == "qmr_update_jacobi":
                el("W", w, 2, np.abs(w))
                red(1, (D["G"] * _r(w, dt)).sum(1), (np.abs(D["G"]) * np.abs(w)).sum(1), 2)
            else:
                el("D", _r(w, dt) + _col(beta) * D["D"], 4, np.abs(w) + np.abs(_col(beta) * D["D"]))
    elif ep in ("axpy_proj_dot", "axpy_proj_dot_jacobi", "axpy_proj_dot_jacobi_dev"):
        alpha, xr = s["alpha"], s["xr"]
        if ep == "axpy_proj_dot_jacobi_dev":
            alpha, bad = qmr_alpha(s["tri"], s["rho_prev"], nx)
            assert not bad.any(), cid
            xr = s["tri"][:nx]
        g, Sg, o, So = ref_proj(dt, alpha, xr, D["W"], D["X"], D["G"])
        el("G", g, 4, Sg)
        red(0, o, So, 4)
        if ep != "axpy_proj_dot":
            den = ref_den(D["diag"][0], s["shift0"], s["mind"])
            gt = _r(g, dt)
            red(1, (gt * _r(gt / den, dt)).sum(1), (Sg * Sg / np.abs(den)).sum(1), 6)
    elif ep == "jacobi":
        den = ref_den(D["diag"][0].real, s["shift0"], s["mind"])
        with np.errstate(invalid="ignore"):
            v, y = D["x"] / den, _take(ops, got, "y")
        keep = np.ones(m, bool)
        if c.get("nanrow"):
            keep[m // 2] = False
            bad = y[:, m // 2]
            if not (np.isnan(bad.real).all() and (not is_z(dt) or np.isnan(bad.imag).all())):
                rep.fails.append(f"{cid}: the row with a NaN diagonal entry is not NaN in y: {bad}")
        for part in (("real", "imag") if is_z(dt) else ("real",)):
            ref = getattr(v, part)[:, keep]
            rep.cmp(f"{cid} y.{part}", getattr(y, part)[:, keep], ref, bound_elem(rdt, 2, np.abs(ref)))
    else:
        raise ValueError(ep)


def _sequence(side, c, ops, s, d):
    """the unfused calls the header promises bit-for-bit equality with: {operand: flat array} of what they leave, or None"""
    ep, dt, m, nx = c["ep"], c["dt"], c["m"], c["nx"]
    neg = lambda v: -np.asarray(v)
    if ep in ("axpy_dot", "axpy_dot_self"):
        b = Bed(side, ops)
        assert call("axpy", side, b, s, m, nx, dt) == 0
        if ep == "axpy_dot":
            rc = side.lib.hipk_pair_dots(side.ctx, dt, m, b.p("Z"), b.ld("Z"), b.p("Y"), b.ld("Y"), nx, b.p("out"))
        else:
            rc = side.lib.hipk_pair_dots(side.ctx, dt, m, b.p("Y"), b.ld("Y"), b.p("Y"), b.ld("Y"), nx, b.p("out"))
        assert rc == 0
        g = b.get()
        return {"Y": g["Y"], "out": g["out"]}
    if ep in ("axpy_proj_dot", "axpy_proj_dot_jacobi"):
        if ep == "axpy_proj_dot_jacobi":                                    # G as hipk_axpy_proj_dot leaves it
            b = Bed(side, ops)
            assert call("axpy_proj_dot", side, b, s, m, nx, dt) == 0
            g = b.get()
            return {"G": g["G"], "~out": g["out"]}
        o2 = dict(ops, T=_scratch(c, ops["W"], d["W"]))                     # 1. W copied to a scratch panel
        b = Bed(side, o2)
        rc1 = side.lib.hipk_axpy_cols(side.ctx, dt, m, _da(neg(s["xr"])), b.p("X"), b.ld("X"), b.p("T"), b.ld("T"), nx)
        rc2 = side.lib.hipk_axpy_cols(side.ctx, dt, m, _da(neg(s["alpha"])), b.p("T"), b.ld("T"), b.p("G"), b.ld("G"), nx)
        assert rc1 == 0 and rc2 == 0
        return {"G": b.get()["G"]}
    if ep == "qmr_update_jacobi":
        b = Bed(side, ops)
        assert call("qmr_update", side, b, s, m, nx, dt) == 0 and jacobi(side, b, s, m, nx, dt, "G", "W") == 0
        g = b.get()
        return {"Delta": g["Delta"], "Sol": g["Sol"], "W": g["W"], "~out": g["out"]}
    if ep == "qmr_update_dir":
        o2 = dict(ops, T=_scratch(c, ops["G"], None))
        b = Bed(side, o2)
        assert call("qmr_update", side, b, s, m, nx, dt) == 0 and jacobi(side, b, s, m, nx, dt, "G", "T") == 0
        assert side.lib.hipk_axpy_cols(side.ctx, dt, m, _da(s["beta"]), b.p("D"), b.ld("D"), b.p("T"), b.ld("T"), nx) == 0
        g = b.get()
        new_d = ops["D"].host.copy()
        new_d[ops["D"].index(range(nx))] = o2["T"].take(g["T"], range(nx))     # the new D must have the bits of scratch
        return {"Delta": g["Delta"], "Sol": g["Sol"], "D": new_d, "~out": g["out"]}
    if ep in DEV_EPS:                                                        # the host-coefficient twin, coefficients from numpy
        alpha, bad = qmr_alpha(s["tri"], s["rho_prev"], nx)
        s2 = dict(s, alpha=alpha, xr=np.asarray(s["tri"][:nx]))
        s2["gam"], s2["eta"], s2["beta"] = qmr_coeffs(s["ggr"], alpha, s["rho_prev"], s["tau_prev"], s["theta_prev"], nx)
        b = Bed(side, ops)
        assert call(ep[:-4], side, b, s2, m, nx, dt) == 0
        g = b.get()
        return {k: g[k] for k in EPS[ep][6] + ("out",)}
    return None


def _run_case(side, c, rep):
    ep, dt, m, nx = c["ep"], c["dt"], c["m"], c["nx"]
    cid = case_id(c)
    ops, s, d = build(c)
    b = Bed(side, ops)
    rc = call(ep, side, b, s, m, nx, dt)
    assert rc == 0, f"{cid}: rc = {rc}"
    got = b.fetch(rep, cid)
    _check_ref(rep, cid, c, ops, s, d, got)
    seq = _sequence(side, c, ops, s, d)
    if seq:
        for k, v in seq.items():
            if k.startswith("~"):          # no bit equality promised for this reduction: the bound above covers it; say whether the bits agree
                n = int((_bits(got[k[1:]])[ops["out"].off:ops["out"].off + nx] == _bits(v)[ops["out"].off:ops["out"].off + nx]).all())
                rep.agree = getattr(rep, "agree", 0) + n
                rep.agree_of = getattr(rep, "agree_of", 0) + 1
            else:
                rep.same_bits(f"{cid} {k}: fused against the separate calls", got[k], v)
    if "out" in ops:                       # repeatability of every reduction
        b2 = Bed(side, ops)
        assert call(ep, side, b2, s, m, nx, dt) == 0
        g2 = b2.get()
        for k in ops:
            rep.same_bits(f"{cid} {k}: second run", got[k], g2[k])


def drop_tri(c, rng):
    """tri = [x'w | v'w | v'x] and rho_prev that put every column in its class (x'w stays finite: it is applied to W whatever
    alpha is)"""
    nx = c["nx"]
    tri, rho = rng.standard_normal(3 * nx) * 3.0, np.abs(rng.standard_normal(nx)) + 0.5
    for col, cls in enumerate(c["classes"]):
        if cls == "sigma0":
            tri[nx + col] = tri[col] * tri[2 * nx + col]
        elif cls == "sigma_inf":
            tri[nx + col] = np.inf if col % 2 else -np.inf
        elif cls == "sigma_nan":
            tri[nx + col] = np.nan
        elif cls == "alpha_tiny":
            rho[col] = 1e-20
        elif cls == "rho0":
            rho[col] = 0.0
        elif cls == "alpha_huge":
            tri[2 * nx + col], tri[nx + col] = 0.0, 1e-20
        elif cls == "alpha_inf":
            rho[col] = np.inf
    return tri, rho


def _run_drop(side, c, rep):
    """both launches of a step, as the solver makes them.  Dropped column: G keeps its bits in the first launch; D, Delta, Sol keep
    theirs in the second and dotsol is 0.0.  Live column: both launches equal the host-coefficient launches of that column alone."""
    dt, m, nx = c["dt"], c["m"], c["nx"]
    cid = case_id(c)
    ops, s, d = build(c)
    s["tri"], s["rho_prev"] = drop_tri(c, _rng(c))
    ops["tri"].fill(0, s["tri"])
    alpha, bad = qmr_alpha(s["tri"], s["rho_prev"], nx)
    want = np.array([cls != "live" for cls in c["classes"]])
    assert (bad == want).all(), (cid, bad)
    live = [int(i) for i in np.flatnonzero(~bad)]
    first = {k: ops[k] for k in ("W", "X", "G", "diag", "tri", "out")}
    first["G"].expect(live)
    b = Bed(side, first)
    assert call("axpy_proj_dot_jacobi_dev", side, b, s, m, nx, dt) == 0
    g1 = b.fetch(rep, f"{cid} first launch")
    ggr = ops["out"].take(g1["out"], 0)[0]
    for col in live:                                           # the host-coefficient launch of that column alone
        s1 = dict(s, alpha=alpha, xr=s["tri"][:nx])
        o1 = dict(first, out=small(2))
        b1 = Bed(side, o1)
        assert call("axpy_proj_dot_jacobi", side, b1, s1, m, nx, dt, col=col, n1=1) == 0
        h = b1.get()
        rep.same_bits(f"{cid} G column {col}: device recurrences against host coefficients", ops["G"].take(g1["G"], col), ops["G"].take(h["G"], col))
        rep.same_bits(f"{cid} ggr column {col}", ggr[[col, nx + col]], o1["out"].take(h["out"], 0)[0])
    # second launch on the G and the reductions the first one left
    G2 = _lay(dt, m, nx, c["flavour"], 2)
    assert G2.ld == ops["G"].ld
    G2.host[:] = g1["G"]
    ggr_op = small(2 * nx)
    ggr_op.host[:] = g1["out"]
    dots = small(nx)
    dots.expect(0)
    second = {"D": ops["D"], "Delta": ops["Delta"], "Sol": ops["Sol"], "G": G2, "diag": ops["diag"], "tri": ops["tri"], "ggr": ggr_op, "out": dots}
    for k in ("D", "Delta", "Sol"):
        second[k].expect(live)
    b = Bed(side, second)
    assert call("qmr_update_dir_dev", side, b, s, m, nx, dt) == 0
    g2 = b.fetch(rep, f"{cid} second launch")
    dotsol = dots.take(g2["out"], 0)[0]
    gam, eta, beta = qmr_coeffs(ggr, alpha, s["rho_prev"], s["tau_prev"], s["theta_prev"], nx)
    for col in range(nx):
        if bad[col]:
            if not (dotsol[col] == 0.0 and not np.signbit(dotsol[col])):
                rep.fails.append(f"{cid}: dotsol of the dropped column {col} is {dotsol[col]!r}, not 0.0")
            continue
        s1 = dict(s, gam=gam, eta=eta, beta=beta)
        o1 = dict(second, out=small(1))
        b1 = Bed(side, o1)
        assert call("qmr_update_dir", side, b1, s1, m, nx, dt, col=col, n1=1) == 0
        h = b1.get()
        for k in ("D", "Delta", "Sol"):
            rep.same_bits(f"{cid} {k} column {col}: device recurrences against host coefficients", ops[k].take(g2[k], col), ops[k].take(h[k], col))
        rep.same_bits(f"{cid} dotsol column {col}", dotsol[[col]], o1["out"].take(h["out"], 0)[0])


def _run_rc(side, c, rep):
    """argument errors and empty calls: the documented return code, every operand bit-identical to the upload"""
    ep, dt, kind = c["ep"], c["dt"], c["kind"]
    cid = case_id(c)
    ops, s, d = build(c)
    for op in ops.values():
        op.written[:] = False
    s = dict(s, tri_null=kind == "tri_null", ggr_null=kind == "ggr_null")
    b = Bed(side, ops)
    rc = call(ep, side, b, s, c["m"], 0 if kind == "nx0" else c["nx"], dt)
    if rc != c["rc"]:
        rep.fails.append(f"{cid}: rc = {rc}, the header says {c['rc']}")
    b.fetch(rep, cid)


def run_cases(side_factory, cases):
    """all cases on ONE side object; returns the VReport"""
    rep = VReport()
    rep.agree = rep.agree_of = 0
    side = side_factory()
    try:
        for c in cases:
            rep.flavour = c["flavour"]
            (_run_drop if c["ep"] == "drop" else _run_rc if "kind" in c else _run_case)(side, c, rep)
            rep.ncases += 1
            if c["m"] > 5000 or len(side.keep) > 64:
                _release(side)
    finally:
        _release(side)
        side.close()
    if rep.agree_of:
        rep.notes.append(f"reduction with no promised bit equality agrees bit-wise with the unfused call in {rep.agree} of {rep.agree_of} cases")
    return rep


def groups():
    """[(id, cases)]: one test per (entry point, type), the grid-cap case of each in a group of its own"""
    out = {}
    for c in CASES:
        out.setdefault(f"{c['ep']}-{TNAME[c['dt']]}" + ("-cap" if c.get("cap") else ""), []).append(c)
    for c in DROP:
        out.setdefault(f"drop-{TNAME[c['dt']]}", []).append(c)
    for c in RC:
        out.setdefault(f"rc-{TNAME[c['dt']]}", []).append(c)
    return sorted(out.items())
