"""Cases, operand layouts and high-precision references for the branch-by-branch tests of the CSR ROW-TILE products:
csr_stream_kernel, csr_rows_block_kernel, csr_window_block_kernel (csrc/hipk_sparse.hip, routed by csr_route_of of
csrc/hipk_csr.hip) and zcsr_kernel (csrc/hipk_complex.hip, launched by csr_matvec_z).  tests/test_csr_branches_host.py runs
them on the plain-C oracle, tests/test_csr_branches_gpu.py on the device.  The structure is that of
tests/panel_branch_cases.py, whose Operand / small / gamma / bound_elem / bound_red / Report / run_cases are used here; the
complex conventions are those of tests/complex_branch_cases.py, the tile plan comes through tests/csr_cases.py: tile_plan.

Matrices (matrix(name): plain seeded loops, nothing chosen at run time; at most 5 000 rows and 40 000 nonzeros).  All values
are random, so no row-pattern form is built, all are far too small for the panel-blocked form, and none asks for the sliced
one: every device case asserts hipk_csr_format == 0 and hipk_csr_npatterns == hipk_csr_panels == hipk_csr_sliced == 0.
  band_narrow@n   17 entries per row inside +-32 (so inside +-40): 120 rows per tile, every window <= 184 <= 192 columns,
                  16-bit stream; n = 97, 827, 960, 1000, 1930 rows = 1, 7, 8, 9, 17 tiles (the edges of xcd_tile and of
                  gx = 8 ceil(ntiles / 8): surplus blocks must leave without writing)
  band_narrow_g   band_narrow@1000 created with ncols_global = 2^31 - 1 (a block of a huge block-diagonal operator): the
                  host analysis then gives no 16-bit stream, so the windowed and fused kernels run with C16 = false
  band_wide       17 entries per row inside +-75, 360 rows = 3 full tiles: every window cw has
                  cw 3 <= 1728 < cw 9 <= 3072 < cw 17 (asserted on the plan by the host file)
  short_rows      1 to 3 entries per row next to the diagonal: tiles cut at the 256-row limit (nr == TILE_ROWS), no split
  scattered       3 000 rows, 8 random columns per row: not "windowed", every window about 3 000 wide, 16-bit stream
  rect_far        hipk_csr_create_rect, 300 x 70 000 scattered: no 16-bit stream, input longer than the output
  rect_tall       hipk_csr_create_rect, 5 000 x 300: the tall and narrow shape (the transpose of rect_far would have
                  70 000 rows; the shape is what matters: output longer than the input); every window is at most 300
                  wide, so blocks of 2 to 64 columns take the windowed kernel on a rectangular matrix
  ragged          4 100 rows: empty rows, a row of exactly 2 048 entries (still an LDS tile), rows of 2 049 and 4 000 (tiles
                  of their own: the workgroup reduction), all-empty tiles first, in the middle and last
  zero            hipk_csr_create_rect, 600 x 601, nnz = 0 (a square matrix without entries is one repeated row pattern and
                  gets the row-pattern form; this one stays on the row tiles)
  slab_lo / slab_hi / slab_both   rows [2400, 3000) / [0, 600) / [1000, 1700) of a 3 000-row random band matrix (+-60) with
                  global column numbers: halo only below / only above / on both sides; the first 300 rows of slab_hi are
                  empty (an all-empty tile with a halo); row 300 of slab_both has 2 100 entries over all 3 000 columns (a
                  long row that reaches into both halos)
  slab_far        rows [0, 600) of a band matrix with 70 000 columns whose row 300 reaches column 69 999: a halo slab
                  without the 16-bit stream (the fused product with 32-bit indices)
The complex cases use band_narrow@1000, ragged, slab_both and slab_hi with complex values.

Layout.  Every panel, halo buffer and small array is an Operand [guard | data | guard]; guards, the rows [m, ld) of every
column and spare slots are quiet NaN, outputs are NaN throughout.  ldx, ldy and the two halo strides all differ within a
case.  Flavours: 'even' (even leading dimensions, aligned base) and 'odd' (odd ones, base moved by one element).  After
the call everything the contract does not name as written must be bit-identical, every contracted element finite.  The
kernels multiply clamped loads by zero only at owned entries of x (live data), so the NaN padding is safe by design.
Each product is issued twice into two outputs, which must agree bit for bit (the header promises fixed summation orders).

References (np.longdouble / np.clongdouble, from the contract in include/primme_amd_kernels.h — NOT from oracle/hipk_cpu.c
and not from primme_amd.problems — on the inputs already rounded to T):  column g of row i is served from the owned entries
[x0, x0 + xlen) of x, from lo[g - x0 + halo_lo] below and from hi[g - x0 - xlen] above them.  Each returns the row's sum
of absolute terms S_i.

Bounds (derived, nothing tuned).  u64 = 2^-53, uT the unit round-off of T, gamma(n, u) = n u / (1 - n u):
  * a row of n_i entries accumulated in double (in any order, fused or not: gamma(n_i) S_i) and stored in T (uT |y| <=
    uT S_i), with the factor 2 of panel_branch_cases.py for the reference's own error:   2 (gamma(n_i + 2, u64) + uT) S_i
  * shifted: - shift_c x(i, c) is one more entry: n_i + 1, and |shift_c| |x(i, c)| is added to S_i
  * fused (hipk_csr_matvec_scaled): a = 1 / sqrt(norm2) in longdouble.  xout = round_T(a x) element-wise within
    bound_elem(dt, 1, |a x|) (the device's a carries two double roundings, the product one, the store one).  The product
    is then referred to xout AS STORED for the owned entries (the kernel applies the same expression to the same numbers
    when it gathers them) under the plain row bound.  A halo entry is round_T(a x) of the reference's a; the device's a
    differs by 2 u64, its double product by u64 more, so the two roundings to T agree or are neighbours: 2 uT + 4 u64
    relative to that term.  This is carried as (2 uT + 4 u64) S_halo_i, S_halo_i the halo terms of S_i.
    dot = xout' y of the stored xout and y: bound_red(m, sum |xout_i| |y_i|, dt, n = longest row + 2)
  * complex: a component of a sum of n complex terms is a real sum of 2 n products (complex_branch_cases.py):
    2 (gamma(2 n_i + 2, u64) + uT) S_i per component, S_i = |ar||xr| + |ai||xi| and |ar||xi| + |ai||xr|; a real shift
    adds one entry
No case and no row is left out; the report gives the largest error / bound of every group.

branch_of(case, plan, knobs) restates csr_route_of from the plan of primme_amd_csr_tile_plan; cells_of the per-tile
branches (normal / long-row / all-empty) x (window / gather) x (split 2 / 1) x (local / halo).  Where the device can be
asked the restatement is checked against it (hipk_csr_index_bytes, hipk_csr_format, the halo extents).
"""
import ctypes as C
import functools
import zlib

import numpy as np

from primme_amd import _ffi as F
import checkers
import csr_cases as CC
import panel_branch_cases as P
from panel_branch_cases import Operand, small, gamma, bound_elem, bound_red, Report, GUARD, U64   # noqa: F401
from complex_branch_cases import NPDT, TNAME, absz, sprod, _c

LD, CLD = np.longdouble, np.clongdouble
F64, F32, C64, C32 = F.HIPK_F64, F.HIPK_F32, F.HIPK_C64, F.HIPK_C32
UNIT = {F64: 2.0 ** -53, F32: 2.0 ** -24, C64: 2.0 ** -53, C32: 2.0 ** -24}
RTYPES, ZTYPES = [F64, F32], [C64, C32]
FLAVOURS = ["even", "odd"]
TILE_NNZ, TILE_ROWS, XS_MAX, XS_SMALL, BLOCK = CC.TILE_NNZ, CC.TILE_ROWS, CC.TILE_WINDOW, 1728, 256
NGLOBAL_HUGE = 2 ** 31 - 1


def is_z(dt):
    return dt in (C64, C32)


def bound_row(dt, n, S):
    """a row (a component of a row) of n entries accumulated in double and stored in T: see the module docstring"""
    n = np.asarray(n, np.float64)
    return 2.0 * (gamma((2 * n if is_z(dt) else n) + 2, U64) + UNIT[dt]) * S


# ------------------------------------------------------------------------------------------------------------------
# matrices
# ------------------------------------------------------------------------------------------------------------------
class Mat:
    def __init__(self, name, rows, vals_seed, nrows, row0=0, nglobal=None, rect=False, xlen=None):
        self.name, self.nrows, self.row0, self.rect = name, nrows, row0, rect
        assert len(rows) == nrows
        lens = np.array([len(r) for r in rows], dtype=np.int64)
        self.rp = np.zeros(nrows + 1, dtype=np.int32)
        self.rp[1:] = np.cumsum(lens)
        self.ci = (np.concatenate(rows) if lens.sum() else np.zeros(0)).astype(np.int32)
        rng = np.random.default_rng(vals_seed)
        nnz = len(self.ci)
        # magnitudes over two decades: an error relative to the largest row would hide a wrong term of a small one
        mag = 10.0 ** rng.uniform(-1.0, 1.0, size=nnz)
        self.va = rng.standard_normal(nnz) * mag
        self.vb = rng.standard_normal(nnz) * mag[::-1]          # imaginary parts of the complex twin
        self.x0 = 0 if rect else row0
        self.xlen = xlen if rect else nrows
        self.nglobal = nglobal if nglobal is not None else max(row0 + nrows, self.x0 + self.xlen)
        self.lens = lens
        self.rowid = np.repeat(np.arange(nrows), lens)

    def values(self, dt):
        v = (self.va + 1j * self.vb) if is_z(dt) else self.va
        return np.ascontiguousarray(v.astype(NPDT[dt]))


def _band_rows(nloc, row0, nglobal, per_row, half, seed):
    rng = np.random.default_rng(seed)
    rows = []
    for i in range(nloc):
        g = row0 + i
        lo, hi = max(0, g - half), min(nglobal - 1, g + half)
        rows.append(lo + np.sort(rng.choice(hi - lo + 1, size=min(per_row, hi - lo + 1), replace=False)))
    return rows


def _scatter_rows(counts, ncols, seed):
    rng = np.random.default_rng(seed)
    return [np.sort(rng.choice(ncols, size=int(c), replace=False)) for c in counts]


@functools.lru_cache(maxsize=None)
def _global_band():
    return _band_rows(3000, 0, 3000, 9, 60, 41)


@functools.lru_cache(maxsize=None)
def matrix(name):
    if name.startswith("band_narrow@"):
        n = int(name.split("@")[1])
        return Mat(name, _band_rows(n, 0, n, 17, 32, 100 + n), 200 + n, n)
    if name == "band_narrow_g":
        return Mat(name, _band_rows(1000, 0, 1000, 17, 32, 1100), 1200, 1000, nglobal=NGLOBAL_HUGE)
    if name == "band_wide":
        return Mat(name, _band_rows(360, 0, 360, 17, 75, 11), 12, 360)
    if name == "short_rows":
        n, rng, rows = 600, np.random.default_rng(13), []
        for i in range(n):
            near = np.array([j for j in (i - 1, i, i + 1) if 0 <= j < n])
            rows.append(np.sort(rng.choice(near, size=int(rng.integers(1, len(near) + 1)), replace=False)))
        return Mat(name, rows, 14, n)
    if name == "scattered":
        return Mat(name, _scatter_rows([8] * 3000, 3000, 15), 16, 3000)
    if name == "rect_far":
        rng = np.random.default_rng(17)
        rows = _scatter_rows(rng.integers(4, 17, size=300), 70000, 18)
        rows[7] = np.unique(np.concatenate([rows[7], [0, 69999]]))
        return Mat(name, rows, 19, 300, rect=True, xlen=70000)
    if name == "rect_tall":
        rng = np.random.default_rng(20)
        return Mat(name, _scatter_rows(rng.integers(0, 9, size=5000), 300, 21), 22, 5000, rect=True, xlen=300)
    if name == "ragged":
        n, rng = 4100, np.random.default_rng(23)
        counts = rng.integers(0, 7, size=n)
        counts[:300] = 0; counts[1200:1800] = 0; counts[3500:] = 0
        counts[500], counts[501], counts[700], counts[900] = 2048, 0, 2049, 4000
        return Mat(name, _scatter_rows(counts, n, 24), 25, n)
    if name == "zero":
        return Mat(name, [np.zeros(0, dtype=np.int64)] * 600, 26, 600, rect=True, xlen=601)
    if name in ("slab_lo", "slab_hi", "slab_both"):
        row0, m = {"slab_lo": (2400, 600), "slab_hi": (0, 600), "slab_both": (1000, 700)}[name]
        rows = list(_global_band()[row0:row0 + m])
        if name == "slab_hi":
            rows[:300] = [np.zeros(0, dtype=np.int64)] * 300           # an all-empty tile in a slab with a halo
        if name == "slab_both":
            rows[300] = np.sort(np.random.default_rng(27).choice(3000, size=2100, replace=False))
        return Mat(name, rows, 28 + row0, m, row0=row0, nglobal=3000)
    if name == "slab_far":
        rows = _band_rows(600, 0, 70000, 9, 60, 31)
        rows[300] = np.unique(np.concatenate([rows[300], np.random.default_rng(32).choice(70000, size=40, replace=False), [69999]]))
        return Mat(name, rows, 33, 600, row0=0, nglobal=70000)
    raise ValueError(name)


@functools.lru_cache(maxsize=None)
def plan_of(name, real=True):
    """the host analysis the device object is built from (csrc/csr_tools.c), through the CPU checker library"""
    M = matrix(name)
    return CC.tile_plan(checkers.load_hostcheck(), M.rp, M.ci, M.values(F64 if real else C64), row0=M.row0, x0=M.x0, xlen=M.xlen,
                        ncols_global=M.nglobal, real=real)


# ------------------------------------------------------------------------------------------------------------------
# references
# ------------------------------------------------------------------------------------------------------------------
def _row_sums(M, terms):
    """terms (w, nnz) -> (w, nrows): the entries of a row added up (reduceat over the non-empty rows: the entries of the
    empty ones in between are none, so consecutive starts bound exactly one row each)"""
    out = np.zeros((terms.shape[0], M.nrows), terms.dtype)
    ne = np.flatnonzero(M.lens)
    if len(ne):
        out[:, ne] = np.add.reduceat(terms, M.rp[:-1][ne].astype(np.int64), axis=1)
    return out


def _gather(M, plan, X, lo, hi):
    """x at every nonzero's column, from the contract: owned entries, else the halo buffers; (w, nnz) in the type of X,
    and the mask of the entries that came out of a halo"""
    xx = np.concatenate([lo, X, hi], axis=1)
    idx = M.ci.astype(np.int64) - M.x0 + plan.halo_lo
    assert xx.shape[1] == plan.halo_lo + M.xlen + plan.halo_hi and (len(idx) == 0 or (idx.min() >= 0 and idx.max() < xx.shape[1]))
    l = M.ci.astype(np.int64) - M.x0
    return xx[:, idx], (l < 0) | (l >= M.xlen)


def ref_matvec(M, plan, dt, X, lo, hi, shift=None):
    """y(i, c) = sum_j a_ij x(j, c) [- shift_c x(i, c)]: (y, S, n) with S the sums of absolute terms (a complex S holds
    the two components') and n the entries per row"""
    xg, _ = _gather(M, plan, X, lo, hi)
    n = M.lens.astype(np.float64)
    if is_z(dt):
        a, xg = _c(M.values(dt)), _c(xg)
        y, S = _row_sums(M, a[None, :] * xg), _row_sums(M, sprod(a[None, :], absz(xg)))
        if shift is not None:
            s = np.asarray(shift, LD)[:, None]
            y, S, n = y - s * _c(X), S + np.abs(s) * absz(X), n + 1
        return y, S, n
    a, xg = np.asarray(M.values(dt), LD), np.asarray(xg, LD)
    y, S = _row_sums(M, a[None, :] * xg), _row_sums(M, np.abs(a)[None, :] * np.abs(xg))
    if shift is not None:
        s = np.asarray(shift, LD)[:, None]
        y, S, n = y - s * np.asarray(X, LD), S + np.abs(s) * np.abs(np.asarray(X, LD)), n + 1
    return y, S, n


def ref_scaled(M, plan, dt, x, lo, hi, norm2, xout_stored):
    """a, a x (for xout's own bound), then y = A [xout as stored | round_T(a halo)]: (ax, y, S, S_halo)"""
    a = LD(1) / np.sqrt(LD(norm2)) if norm2 is not None else LD(1)
    ax = a * np.asarray(x, LD)
    rnd = lambda v: np.asarray(v, LD).astype(NPDT[dt])
    xg, halo = _gather(M, plan, np.asarray(xout_stored, NPDT[dt])[None, :], rnd(a * np.asarray(lo, LD)), rnd(a * np.asarray(hi, LD)))
    va, xg = np.asarray(M.values(dt), LD), np.asarray(xg, LD)
    t = np.abs(va)[None, :] * np.abs(xg)
    return ax, _row_sums(M, va[None, :] * xg)[0], _row_sums(M, t)[0], _row_sums(M, np.where(halo[None, :], t, 0))[0]


# ------------------------------------------------------------------------------------------------------------------
# the routing, restated
# ------------------------------------------------------------------------------------------------------------------
KNOBS = {
    None: dict(env={}),
    "nt": dict(env={"HIPK_SPMV_NT": "1"}, nt=1),
    "nc1": dict(env={"HIPK_SPMM_NC": "1", "HIPK_NO_WINDOW": "1"}, nc=1, no_window=True),
    "nocol16_big": dict(env={"HIPK_SPMM_NO_COL16": "1", "HIPK_SPMM_BIG_WINDOW": "1"}, no_col16=True, big_window=True),
    "even_nosplit": dict(env={"HIPK_SPMM_EVEN_STRIDE": "1", "HIPK_SPMM_NO_SPLIT": "1"}, even_stride=True, no_split=True),
}


def _xst(w, K):
    return w if K.get("even_stride") else (w | 1)


def branch_of(c, plan, knobs=None):
    """The instantiation of every launch the documented routing makes for a case.  THIS MIRRORS csr_route_of of
    csrc/hipk_csr.hip (and csr_matvec_z / hipk_z_csr_matvec for the complex types): when the routing changes, this function
    and the tables change with it.  knobs: a key of KNOBS (the environment csr_knobs() read in that process)."""
    K, t, w, ep = KNOBS[knobs], TNAME[c["dt"]], c["w"], c["ep"]
    if c.get("rc"):
        return []                                               # declined before any launch
    if is_z(c["dt"]):
        return [("zcsr_kernel", t, 1 if n == 1 else 2 if n == 2 else 4) for n in [min(64, w - c0) for c0 in range(0, w, 64)]]
    c16 = plan.col16 is not None and not K.get("no_col16")
    local = plan.halo_lo == 0 and plan.halo_hi == 0
    if ep != "scaled" and local and w <= 64 and ((plan.windowed and w >= 2 and not K.get("no_window")) or ep == "shifted"):
        small_buf = not K.get("big_window") and plan.cw_max * _xst(w, K) <= XS_SMALL
        return [("csr_window_block_kernel", t, 2 if w <= 2 else 4, "XS_SMALL" if small_buf else "XS_MAX", c16)]
    if ep == "scaled" or (w == 1 and K.get("nc", 0) == 0):
        return [("csr_stream_kernel", t, ep == "scaled", c16, K.get("nt", -1) > 0)]      # (by size: never at these sizes)
    nc = K.get("nc", 0)
    return [("csr_rows_block_kernel", t, 1 if nc == 1 else 2 if (nc == 2 or (nc == 0 and w <= 2)) else 4)]


def index_bytes_of(plan, knobs=None):
    """hipk_csr_index_bytes: what the route of the one-column plain product reads per index"""
    b = branch_of(dict(ep="matvec", dt=F64, w=1), plan, knobs)[0]
    return 2 if (b[0] != "csr_rows_block_kernel" and b[3 if b[0] == "csr_stream_kernel" else 4]) else 4


def cells_of(c, plan, knobs=None):
    """(cells, marks): the per-tile branches a case passes through, as (normal | long | empty, window | gather, split,
    local | halo), and the other edges it meets"""
    K, cells, marks = KNOBS[knobs], set(), set()
    halo = "local" if plan.halo_lo == 0 and plan.halo_hi == 0 else "halo"
    for b in branch_of(c, plan, knobs):
        kern = b[0]
        w = c["w"] if not is_z(c["dt"]) else min(c["w"], 64)
        for k in range(plan.ntiles):
            r0, r1, p0, p1 = (int(v) for v in plan.info[k])
            nz, nr, cw = p1 - p0, r1 - r0, int(plan.win[k, 1])
            kind = "long" if nz > TILE_NNZ else "empty" if nz == 0 else "normal"
            wg, split = "gather", 1
            if kern == "csr_window_block_kernel" and kind != "long":
                xs = XS_SMALL if b[3] == "XS_SMALL" else XS_MAX
                if cw > 0 and cw * _xst(w, K) <= xs:
                    wg = "window"
                ngroups = -(-w // b[2])
                split = 2 if (2 * nr * ngroups <= BLOCK and not K.get("no_split")) else 1
            cells.add((kind, wg, split, halo))
            if nr == TILE_ROWS and kern != "csr_stream_kernel" and kern != "zcsr_kernel":
                marks.add(("nr==TILE_ROWS", kern))
            if kind == "long":
                marks.add(("long", kern, c["ep"], halo))
        marks.add(("ntiles", plan.ntiles))
        if plan.ntiles % 8:
            marks.add(("surplus blocks", kern))
    if is_z(c["dt"]) and c["w"] > 64 and not c.get("rc"):
        marks.add(("two launches", halo))
    return cells, marks


AXES = [("normal", "long", "empty"), ("window", "gather"), (2, 1), ("local", "halo")]
# the cells of the grid no product can reach, by name and with the reason
UNREACHABLE = {}
for _kind in AXES[0]:
    for _wg in AXES[1]:
        for _sp in AXES[2]:
            if _wg == "window" or _sp == 2:
                UNREACHABLE[(_kind, _wg, _sp, "halo")] = ("a matrix with halos is never routed to the windowed kernel, and only that kernel stages "
                                                          "a window or shares a row between two lanes")
for _sp in AXES[2]:
    UNREACHABLE[("long", "window", _sp, "local")] = "a tile of more than TILE_NNZ entries is one row reduced by the whole workgroup from global memory"
    UNREACHABLE[("empty", "window", _sp, "local")] = "the host analysis gives a tile without entries the window {0, 0}"
UNREACHABLE[("long", "gather", 2, "local")] = "the workgroup reduction of a long row has no two-lane split"
REACHABLE = {(a, b, s, h) for a in AXES[0] for b in AXES[1] for s in AXES[2] for h in AXES[3]} - set(UNREACHABLE)


def wanted_instantiations():
    want = set()
    for t in ("f64", "f32"):
        want |= {("csr_stream_kernel", t, fu, c16, nt) for fu in (False, True) for c16 in (False, True) for nt in (False, True)}
        want |= {("csr_rows_block_kernel", t, nc) for nc in (1, 2, 4)}
        want |= {("csr_window_block_kernel", t, nc, xs, c16) for nc in (2, 4) for xs in ("XS_SMALL", "XS_MAX") for c16 in (False, True)}
    for t in ("c64", "c32"):
        want |= {("zcsr_kernel", t, nc) for nc in (1, 2, 4)}
    return want


WANTED_MARKS = ({("ntiles", n) for n in (1, 7, 8, 9, 17)} | {("nr==TILE_ROWS", k) for k in ("csr_rows_block_kernel", "csr_window_block_kernel")} |
                {("surplus blocks", k) for k in ("csr_stream_kernel", "csr_rows_block_kernel", "csr_window_block_kernel", "zcsr_kernel")} |
                {("long", "csr_window_block_kernel", "shifted", "local"), ("long", "csr_stream_kernel", "scaled", "local"),
                 ("long", "csr_stream_kernel", "scaled", "halo"), ("long", "csr_stream_kernel", "matvec", "halo"),
                 ("long", "csr_rows_block_kernel", "matvec", "halo"), ("long", "csr_rows_block_kernel", "matvec", "local"),
                 ("long", "zcsr_kernel", "matvec", "halo"), ("long", "zcsr_kernel", "shifted", "local"), ("two launches", "halo"),
                 ("two launches", "local")})


# ------------------------------------------------------------------------------------------------------------------
# case tables (static)
# ------------------------------------------------------------------------------------------------------------------
MATVEC = [("band_narrow@97", [1, 2, 8]), ("band_narrow@827", [2, 3]), ("band_narrow@960", [4, 64]), ("band_narrow@1000", [1, 5, 9, 16, 65]),
          ("band_narrow@1930", [2, 8]), ("band_narrow_g", [1, 2, 8]), ("band_wide", [2, 3, 8, 9, 16, 64, 65]), ("short_rows", [1, 2, 4, 65]),
          ("scattered", [1, 2, 3, 5, 16, 65]), ("rect_far", [1, 2, 5, 9]), ("rect_tall", [1, 3, 65]), ("ragged", [1, 2, 3, 8, 64, 65]),
          ("zero", [1, 3]), ("slab_lo", [1, 2, 4]), ("slab_hi", [1, 3, 9]), ("slab_both", [1, 2, 5, 65]), ("slab_far", [1])]
SHIFTED = [("band_narrow@1000", [1, 2, 5, 8, 64]), ("band_narrow@97", [1, 8]), ("band_narrow_g", [1, 5]), ("band_wide", [2, 8, 64]),
           ("short_rows", [1, 5]), ("scattered", [1, 2, 8]), ("ragged", [1, 2, 5, 64])]
# declined: 1 and y untouched (a halo slab, a rectangular matrix, 65 columns, no shifts)
SHIFTED_RC = [("slab_both", 2, {}), ("rect_far", 2, {}), ("rect_tall", 1, {}), ("band_narrow@97", 65, {}), ("band_narrow@97", 2, {"noshift": True})]
SCALED = ["band_narrow@1000", "band_narrow_g", "short_rows", "ragged", "slab_lo", "slab_both", "slab_far"]
ZMATVEC = [("band_narrow@1000", [1, 2, 3, 5, 64, 65]), ("ragged", [1, 2, 3, 5, 65]), ("slab_both", [1, 2, 3, 65]), ("slab_hi", [2])]
ZSHIFTED = [("band_narrow@1000", [1, 2, 5, 64]), ("ragged", [1, 2, 5])]
ZSHIFTED_RC = [("band_narrow@1000", 65, {}), ("slab_both", 2, {})]
# the environment-knob variants (one child process each on the device)
KNOB_CASES = {
    "nt": [("matvec", "band_narrow@1000", 1, {}), ("matvec", "rect_far", 1, {}), ("matvec", "slab_both", 1, {}), ("matvec", "zero", 1, {})] +
          [("scaled", m, 1, dict(norm2=True, fin=f)) for m in ("band_narrow@1000", "ragged", "slab_far", "band_narrow_g") for f in (0, 4)],
    "nc1": [("matvec", "scattered", w, {}) for w in (1, 2, 5)] + [("matvec", "ragged", w, {}) for w in (1, 3)] +
           [("matvec", "slab_both", 3, {}), ("matvec", "band_narrow@1000", 2, {}), ("matvec", "band_narrow@1000", 8, {}),
            ("matvec", "short_rows", 1, {}), ("matvec", "rect_far", 2, {})],
    "nocol16_big": [("matvec", "band_narrow@1000", w, {}) for w in (1, 2, 8)] + [("matvec", "band_wide", 8, {}), ("matvec", "band_narrow@97", 3, {})] +
                   [("shifted", "band_narrow@1000", w, {}) for w in (1, 5)] + [("shifted", "scattered", 2, {}), ("scaled", "band_narrow@1000", 1, dict(norm2=True, fin=0))],
    "even_nosplit": [("matvec", "band_narrow@1000", w, {}) for w in (2, 4, 8)] + [("matvec", "band_narrow@97", 2, {}), ("matvec", "band_wide", 2, {}),
                    ("matvec", "band_wide", 8, {}), ("matvec", "band_wide", 16, {}), ("shifted", "band_narrow@1000", 1, {}), ("shifted", "ragged", 2, {})],
}


def _cases():
    out = []
    for dt in RTYPES:
        for fl in FLAVOURS:
            out += [dict(ep="matvec", dt=dt, mat=m, w=w, flavour=fl) for m, ws in MATVEC for w in ws]
            out += [dict(ep="shifted", dt=dt, mat=m, w=w, flavour=fl) for m, ws in SHIFTED for w in ws]
            out += [dict(ep="shifted", dt=dt, mat=m, w=w, flavour=fl, rc=1, **kw) for m, w, kw in SHIFTED_RC]
            out += [dict(ep="scaled", dt=dt, mat=m, w=1, flavour=fl, norm2=n2, fin=fin) for m in SCALED for n2 in (True, False) for fin in (0, 4)]
            out.append(dict(ep="scaled", dt=dt, mat="band_narrow@97", w=1, flavour=fl, norm2=True, fin=0, rc=-1, alias=True))
    for dt in ZTYPES:
        for fl in FLAVOURS:
            out += [dict(ep="matvec", dt=dt, mat=m, w=w, flavour=fl) for m, ws in ZMATVEC for w in ws]
            out += [dict(ep="shifted", dt=dt, mat=m, w=w, flavour=fl) for m, ws in ZSHIFTED for w in ws]
            out += [dict(ep="shifted", dt=dt, mat=m, w=w, flavour=fl, rc=1, **kw) for m, w, kw in ZSHIFTED_RC]
    for kn, lst in KNOB_CASES.items():
        for di, dt in enumerate(RTYPES):
            out += [dict(ep=ep, dt=dt, mat=m, w=w, flavour=FLAVOURS[(i + di) % 2], knobs=kn, **kw) for i, (ep, m, w, kw) in enumerate(lst)]
    return out


CASES = _cases()

# What the plain-C oracle cannot tell apart, by name and with the reason (nothing is skipped: the cases run on it as they are):
ORACLE_SAME = {
    "scaled/fin": "hipk_set_inkernel_fin exists only in the device library; the oracle has one second stage, so both settings run the same loop",
    "knobs": "the HIPK_SPMV_* / HIPK_SPMM_* knobs select between device kernels; the oracle has one loop per product",
}


def case_id(c, flavour=True):
    keys = [k for k in ("w", "norm2", "fin", "rc", "noshift", "alias", "knobs") if k in c] + (["flavour"] if flavour else [])
    return f"{c['ep']}[{TNAME[c['dt']]},{c['mat']}," + ",".join(f"{k}={c[k]}" for k in keys) + "]"


def groups(knobs=False):
    """[(id, cases)]: one test per (entry point, type, flavour); with knobs=True per (knob set, type) instead"""
    out = {}
    for c in CASES:
        if bool(c.get("knobs")) != knobs:
            continue
        key = f"knob-{c['knobs']}-{TNAME[c['dt']]}" if knobs else f"{c['ep']}-{TNAME[c['dt']]}-{c['flavour']}"
        out.setdefault(key, []).append(c)
    return sorted(out.items())


def check_knob_cases(knobs):
    """the instantiations and cells a knob set is there for, through branch_of / cells_of with that knob set"""
    cases = [c for c in CASES if c.get("knobs") == knobs]
    inst, cells = set(), set()
    for c in cases:
        plan = plan_of(c["mat"])
        inst |= set(branch_of(c, plan, knobs))
        cells |= cells_of(c, plan, knobs)[0]
    both = ("f64", "f32")
    if knobs == "nt":
        assert inst == {("csr_stream_kernel", t, fu, c16, True) for t in both for fu in (False, True) for c16 in (False, True)}, inst
    elif knobs == "nc1":
        assert inst == {("csr_rows_block_kernel", t, 1) for t in both}, inst
        assert {c["w"] for c in cases} >= {1, 2, 5} and any(plan_of(c["mat"]).windowed and c["w"] >= 2 for c in cases)      # HIPK_NO_WINDOW
        assert cells == {(a, "gather", 1, h) for a in AXES[0] for h in AXES[3]} - {("empty", "gather", 1, "halo")}, cells
    elif knobs == "nocol16_big":
        assert {x for x in inst if x[0] == "csr_window_block_kernel"} == {("csr_window_block_kernel", t, nc, "XS_MAX", False) for t in both for nc in (2, 4)}, inst
        assert inst - {x for x in inst if x[0] == "csr_window_block_kernel"} == {("csr_stream_kernel", t, fu, False, False) for t in both for fu in (False, True)}
        assert any(plan_of(c["mat"]).cw_max * 9 <= XS_SMALL for c in cases)                  # XS_MAX on windows that fit the small buffer
    elif knobs == "even_nosplit":
        assert all(x[0] == "csr_window_block_kernel" for x in inst) and {x[3] for x in inst} == {"XS_SMALL", "XS_MAX"}, inst
        assert all(s == 1 for (_, _, s, _) in cells) and {wg for (_, wg, _, _) in cells} == {"window", "gather"}, cells
        # the even stride changes which buffer and which branch a width takes: 8 columns of band_wide fit the window at stride 8
        wide = plan_of("band_wide")
        assert wide.cw_max * 8 <= XS_MAX and cells_of(dict(ep="matvec", dt=F64, mat="band_wide", w=8), wide, knobs)[0] == {("normal", "window", 1, "local")}
    else:
        raise ValueError(knobs)


# ------------------------------------------------------------------------------------------------------------------
# runners
# ------------------------------------------------------------------------------------------------------------------
def _lds(flavour, lens):
    """distinct leading dimensions for operands of the given lengths: even ones / odd ones, each longer than its operand"""
    used, out = set(), []
    for i, n in enumerate(lens):
        ld = n + 2 * (i + 1)
        ld += (ld % 2) if flavour == "even" else (1 - ld % 2)
        while ld in used:
            ld += 2
        used.add(ld)
        out.append(ld)
    return out


def _rand(rng, shape, dt):
    z = rng.standard_normal(shape) * np.linspace(1.0, 3.0, shape[0])[:, None]
    if is_z(dt):
        z = z + 1j * rng.standard_normal(shape) * np.linspace(2.0, 0.5, shape[0])[:, None]
    return z.astype(NPDT[dt])


@functools.lru_cache(maxsize=None)
def _inputs(ep, dt, mat, w, noshift, declined=False):
    """the data of a case and its reference: the same for both flavours and both sides, computed once, never changed"""
    M, plan = matrix(mat), plan_of(mat, not is_z(dt))
    rng = np.random.default_rng(zlib.crc32(f"{ep},{dt},{mat},{w}".encode()))
    X, lo, hi = _rand(rng, (w, M.xlen), dt), _rand(rng, (w, plan.halo_lo), dt), _rand(rng, (w, plan.halo_hi), dt)
    shift = None if (ep != "shifted" or noshift) else np.ascontiguousarray(np.linspace(-1.7, 2.3, w) + 0.01 * rng.standard_normal(w))
    norm2 = float(rng.uniform(0.5, 9.0))
    ref = ref_matvec(M, plan, dt, X, lo, hi, shift) if ep != "scaled" and not declined else None
    for a in (X, lo, hi):
        a.setflags(write=False)
    return X, lo, hi, shift, norm2, ref


def _declare(lib):
    for name in ("hipk_csr_index_bytes", "hipk_csr_panels", "hipk_csr_format", "hipk_csr_npatterns", "hipk_csr_sliced"):
        if hasattr(lib, name):
            getattr(lib, name).argtypes, getattr(lib, name).restype = [C.c_void_p], C.c_int
    if hasattr(lib, "hipk_set_inkernel_fin"):
        lib.hipk_set_inkernel_fin.argtypes, lib.hipk_set_inkernel_fin.restype = [C.c_int], C.c_int


def _create(side, c, M, plan):
    """the operator; on the device: served by the row tiles and by nothing else, and routed as branch_of says"""
    dt, cid, A, va = c["dt"], case_id(c), C.c_void_p(), M.values(c["dt"])
    vp = lambda a: a.ctypes.data_as(C.c_void_p)
    if M.rect:
        rc = side.lib.hipk_csr_create_rect(side.ctx, dt, M.nrows, M.xlen, vp(M.rp), vp(M.ci), vp(va), C.byref(A))
    else:
        rc = side.lib.hipk_csr_create(side.ctx, dt, M.nrows, M.nglobal, M.row0, vp(M.rp), vp(M.ci), vp(va), C.byref(A))
    assert rc == 0 and A, f"{cid}: create rc = {rc}"
    assert (side.lib.hipk_csr_halo_lo(A), side.lib.hipk_csr_halo_hi(A)) == (plan.halo_lo, plan.halo_hi), cid
    _declare(side.lib)
    if side.name == "hip" and hasattr(side.lib, "hipk_csr_format"):
        form = (side.lib.hipk_csr_format(A), side.lib.hipk_csr_npatterns(A), side.lib.hipk_csr_panels(A), side.lib.hipk_csr_sliced(A))
        assert form == (0, 0, 0, 0), f"{cid}: not served by the row tiles alone: (format, patterns, panels, sliced) = {form}"
        if not is_z(dt):
            assert side.lib.hipk_csr_index_bytes(A) == index_bytes_of(plan, c.get("knobs")), cid
    return A


def _halo_ops(side, c, plan, npdt, lo, hi, ld_lo, ld_hi, w):
    """the halo buffers through hipk_csr_set_halo_ld, strides larger than the halos; an absent side is NULL"""
    sh = 1 if c["flavour"] == "odd" else 0
    ops = []
    for data, n, ld in ((lo, plan.halo_lo, ld_lo), (hi, plan.halo_hi, ld_hi)):
        if n:
            op = Operand(npdt, n, w, ld, sh)
            op.fill(range(w), data)
            ops.append((op, side.arr(op.host)))
        else:
            ops.append((None, None))
    return ops


def _set_halo(side, A, ops):
    (lo, tlo), (hi, thi) = ops
    assert side.lib.hipk_csr_set_halo_ld(A, lo.base(side, tlo) if lo else None, lo.ld if lo else 0, hi.base(side, thi) if hi else None, hi.ld if hi else 0) == 0


def _cmp_rows(rep, what, dt, got, ref, S, n, extra=None):
    """every row of every column against its own bound; a complex result by components"""
    if is_z(dt):
        ref, S = np.asarray(ref, CLD), np.asarray(S, CLD)
        rep.cmp(what + " (re)", got.real, ref.real, bound_row(dt, n, S.real))
        rep.cmp(what + " (im)", got.imag, ref.imag, bound_row(dt, n, S.imag))
    else:
        rep.cmp(what, got, ref, bound_row(dt, n, S) + (0 if extra is None else extra))


def _run_product(side, c, rep):
    dt, w, cid, npdt = c["dt"], c["w"], case_id(c), np.dtype(NPDT[c["dt"]])
    M, plan = matrix(c["mat"]), plan_of(c["mat"], not is_z(dt))
    want_rc = c.get("rc", 0)
    X, lo, hi, shift, _, ref = _inputs(c["ep"], dt, c["mat"], w, bool(c.get("noshift")), bool(want_rc))
    sh = 1 if c["flavour"] == "odd" else 0
    ldx, ldy, ld_lo, ld_hi = _lds(c["flavour"], [M.xlen, M.nrows, plan.halo_lo, plan.halo_hi])
    assert len({ldx, ldy, ld_lo, ld_hi}) == 4
    xo = Operand(npdt, M.xlen, w, ldx, sh)
    xo.fill(range(w), X)
    ys = [Operand(npdt, M.nrows, w, ldy, sh) for _ in range(2)]
    if want_rc == 0:
        for y in ys:
            y.expect(range(w))
    A = _create(side, c, M, plan)
    try:
        tx, tys = side.arr(xo.host), [side.arr(y.host) for y in ys]
        halos = _halo_ops(side, c, plan, npdt, lo, hi, ld_lo, ld_hi, w)
        _set_halo(side, A, halos)
        for y, ty in zip(ys, tys):
            if c["ep"] == "matvec":
                rc = side.lib.hipk_csr_matvec(A, None, xo.base(side, tx), xo.ld, y.base(side, ty), y.ld, w)
            else:
                rc = side.lib.hipk_csr_matvec_shifted(A, None, xo.base(side, tx), xo.ld, y.base(side, ty), y.ld, w,
                                                      None if shift is None else shift.ctypes.data_as(C.POINTER(C.c_double)))
            assert rc == want_rc, f"{cid}: rc = {rc}, the header says {want_rc}"
        named = [("x", xo, tx), ("y", ys[0], tys[0]), ("y (second call)", ys[1], tys[1])]
        named += [(n, op, t) for n, (op, t) in zip(("halo lo", "halo hi"), halos) if op is not None]
        got = P._finish(side, rep, cid, named)
    finally:
        side.lib.hipk_csr_destroy(A)
    rep.same_bits(f"{cid} y: the same product issued twice", got[1], got[2])
    if want_rc == 0:
        yr, S, n = ref
        _cmp_rows(rep, f"{cid} y", dt, ys[0].take(got[1], range(w)), yr, S, n[None, :])


def _run_scaled(side, c, rep):
    dt, cid, npdt = c["dt"], case_id(c), np.dtype(NPDT[c["dt"]])
    M, plan = matrix(c["mat"]), plan_of(c["mat"])
    X, lo, hi, _, norm2, _ = _inputs("scaled", dt, c["mat"], 1, False)
    want_rc, m = c.get("rc", 0), M.nrows
    sh = 1 if c["flavour"] == "odd" else 0
    ldx, ldo, ldy, ld_lo, ld_hi = _lds(c["flavour"], [m, m, m, plan.halo_lo, plan.halo_hi])
    xo = Operand(npdt, m, 1, ldx, sh)
    xo.fill(0, X)
    n2 = small(1)
    n2.fill(0, [norm2])
    outs = [(Operand(npdt, m, 1, ldo, sh), Operand(npdt, m, 1, ldy, sh), small(1)) for _ in range(2)]
    if want_rc == 0:
        for o in outs:
            for op in o:
                op.expect(0)
    A = _create(side, c, M, plan)
    switch = hasattr(side.lib, "hipk_set_inkernel_fin")          # ORACLE_SAME["scaled/fin"]
    old = side.lib.hipk_set_inkernel_fin(c["fin"]) if switch else None
    try:
        tx, tn = side.arr(xo.host), side.arr(n2.host)
        touts = [tuple(side.arr(op.host) for op in o) for o in outs]
        halos = _halo_ops(side, c, plan, npdt, lo, hi, ld_lo, ld_hi, 1)
        _set_halo(side, A, halos)
        for (xout, y, dot), (txo, ty, td) in zip(outs, touts):
            rc = side.lib.hipk_csr_matvec_scaled(A, side.ctx, xo.base(side, tx), n2.base(side, tn) if c["norm2"] else None,
                                                 xo.base(side, tx) if c.get("alias") else xout.base(side, txo), y.base(side, ty), dot.base(side, td))
            assert rc == want_rc, f"{cid}: rc = {rc}, the header says {want_rc}"
        named = [("x", xo, tx), ("norm2", n2, tn)]
        for i, (o, to) in enumerate(zip(outs, touts)):
            named += [(f"{nm} (call {i + 1})", op, t) for nm, op, t in zip(("xout", "y", "dot"), o, to)]
        named += [(n, op, t) for n, (op, t) in zip(("halo lo", "halo hi"), halos) if op is not None]
        got = P._finish(side, rep, cid, named)
    finally:
        if switch:
            side.lib.hipk_set_inkernel_fin(old)
        side.lib.hipk_csr_destroy(A)
    for j, nm in enumerate(("xout", "y", "dot")):
        rep.same_bits(f"{cid} {nm}: the same product issued twice", got[2 + j], got[5 + j])
    if want_rc:
        return
    xs, yst, dst = outs[0][0].take(got[2], 0)[0], outs[0][1].take(got[3], 0)[0], float(got[4][outs[0][2].off])
    ax, yr, S, Sh = ref_scaled(M, plan, dt, X[0], lo, hi, norm2 if c["norm2"] else None, xs)
    rep.cmp(f"{cid} xout", xs, ax, bound_elem(dt, 1, np.abs(ax)))
    _cmp_rows(rep, f"{cid} y", dt, yst, yr, S, M.lens.astype(np.float64), extra=(2.0 * UNIT[dt] + 4.0 * U64) * Sh)
    xl, yl = np.asarray(xs, LD), np.asarray(yst, LD)
    rep.cmp(f"{cid} dot", dst, (xl * yl).sum(), bound_red(m, (np.abs(xl) * np.abs(yl)).sum(), dt, int(M.lens.max(initial=0)) + 2))


RUNNERS = {"matvec": _run_product, "shifted": _run_product, "scaled": _run_scaled}


def run_cases(side_factory, cases):
    return P.run_cases(side_factory, cases, RUNNERS)
