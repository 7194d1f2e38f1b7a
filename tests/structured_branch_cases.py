"""Cases, operand layouts and high-precision references for the branch-by-branch tests of the forms that serve the ONE-COLUMN
product of structured operators: pat_kernel (csrc/hipk_sparse_pat.hip: plain, fused-scaled, Chebyshev step, each exact and
diagonal-split, local and with halos), pb_matvec_kernel (csrc/hipk_sparse_pb.hip) and stencil_kernel (csrc/hipk_sparse.hip).
tests/test_structured_branches_host.py runs them on the plain-C oracle and carries the coverage assertions,
tests/test_structured_branches_gpu.py runs them on the device.  The structure is that of tests/csr_branch_cases.py, whose
Operand / gamma / bound_elem / bound_red / bound_row / Report / run_cases / _lds / ref_matvec / ref_scaled are used here.

Matrices (matrix(name): plain seeded loops, at most 10 240 rows).  Every value is a dyadic rational out of a small set over two
decades (exact in float, so both types see the same patterns); a row of a lattice operator is decided by its site type alone,
so rows repeat.
  lap1d@n         3-point operator with three different values, n = 1, 2, 511, 512, 513, 1024, 3584, 4096, 4097, 6144, 10240
                  (1, 1, 1, 1, 2, 2, 7, 8, 9, 12, 20 chunks of 512 rows)
  lattice@L       L = 1 .. 8 entries per interior row at the offsets -(L // 2) .. L - L // 2 - 1, not symmetric, two site types
                  that change every 5 rows, 1537 rows (ragged last chunk, odd last row): table widths 3, 3, 3, 5, 5, 7, 7, 8
  ring@2048       periodic 3-point lattice: minoff = -(n - 1), maxoff = n - 1, every chunk `near`
  lap2d@32x64, lap2d@37x41, lap3d@8x8x40     grid operators with a different value per direction, Dirichlet
  holes           lattice@3 with every seventh row empty (1100 rows)
  npat256 / npat257   diagonal matrices with 256 / 257 distinct values (600 rows): the largest table / declined
  row9            a 3-point operator one row of which has 9 entries: declined
  slab:<op>:<row0>:<m>   rows [row0, row0 + m) of a larger operator with GLOBAL columns (hipk_csr_create with row0, halo
                  buffers through hipk_csr_set_halo_ld)
  diag:<matrix>   the diagonal-split twin: the same matrix with a random diagonal, created with HIPK_CSR_DIAG_PATTERNS;
                  diag:nodiag:<matrix> drops the diagonal entry of every eleventh row first (dslot = -1)
  pb_wide, pb_tall, pb_seg   rectangular matrices of the panel-blocked form (hipk_csr_create_rect; HIPK_PB=1 HIPK_PB_KB=8 in
                  the environment of a child process), see PB_* below
  stencil grids   hipk_stencil_create: (1000,), (7, 5), (5, 4, 3), (1, 6), (1, 1, 1), whole and in slabs

Layout, references and bounds are those of tests/csr_branch_cases.py (its module docstring): every operand is
[guard | data | guard] in quiet NaN, outputs NaN throughout, all leading dimensions and halo strides distinct, flavours 'even'
and 'odd' (every base moved by one element: pat_trip_inner moves a pair of rows with one 16-byte buffer access whatever the
alignment), everything the contract does not name as written bit-identical afterwards, every product issued twice and compared
bit for bit.  References are np.longdouble from include/primme_amd_kernels.h on inputs already rounded to T and return the
per-row sums of absolute terms S_i.  Bounds (derived, nothing tuned):
  * a row of n entries:            2 (gamma(n + 2, u64) + uT) S_i                                  (bound_row)
  * fused product:                 exactly as csr_branch_cases.ref_scaled / _run_scaled state it
  * Chebyshev step:                three more terms: bound_row(n + 3) of |cy yk| + |cp yp| + |cx x| + |cw| S_i.  On the oracle
                                   side (no hipk_csr_cheb_step there) the oracle's product, stored in T, followed by the
                                   combination in numpy double takes its place: the stored product is off by uT |cw| S_i more,
                                   the final rounding by uT of the whole, both inside the 2 uT of the bound
  * the stencil:                   a row of 2 dims + 1 entries (its terms are added in double in any order)
  * panel-blocked:                 the per-row bound; it holds in any summation order (lanes add to an LDS slot)
  * deferred tail:                 |t|^2 under bound_red(m, sum t_i^2), xout bit for bit (T)(t / sqrt(|t|^2 as published)), y as
                                   the fused product, t'At under bound_red of the stored xout and y
No case and no row is left out.

pat_info / branch_of / cells_of restate the host side of csrc/hipk_sparse_pat.hip (hipk_pat_build, pat_width, hipk_pat_grid_kind,
the chunk loop of pat_kernel); pb_plan restates hipk_pb_build.  Where the device can be asked the restatement is checked against
it (hipk_csr_format, hipk_csr_npatterns, hipk_csr_pattern_diag, hipk_csr_product_bytes, hipk_csr_panels, the halo extents).
"""
import ctypes as C
import functools
import zlib

import numpy as np

from primme_amd import _ffi as F
import csr_branch_cases as CB
import panel_branch_cases as P
from panel_branch_cases import Operand, small, gamma, bound_elem, bound_red, Report, U64   # noqa: F401
from csr_branch_cases import bound_row, UNIT, _lds, FLAVOURS, RTYPES, F64, F32, LD
from complex_branch_cases import NPDT, TNAME

CHUNK = 512                          # HIPK_BLOCK * 2 rows with HIPK_PAT_RPL = 1
PAT_MAXLEN, PAT_MAXPAT = 8, 256
DIAG_PATTERNS = 1                    # HIPK_CSR_DIAG_PATTERNS
VALSET = np.array([0.125, 0.1875, 0.25, 0.375, 0.5, 0.625, 0.75, 1.0, 1.25, 1.5, 2.0, 2.5, 3.0, 4.0, 5.0, 6.0, 8.0, 10.0, 12.0])


# ------------------------------------------------------------------------------------------------------------------
# matrices
# ------------------------------------------------------------------------------------------------------------------
class Mat:
    """CSR rows [row0, row0 + nrows) with global columns; halo extents from the contract (the columns below / above the owned
    entries [x0, x0 + xlen) of x).  Stands for its own `plan` in csr_branch_cases.ref_matvec / ref_scaled (halo_lo, halo_hi)."""

    def __init__(self, name, rows, vals, row0=0, nglobal=None, rect=False, xlen=None, diag=False):
        self.name, self.nrows, self.row0, self.rect, self.diag = name, len(rows), row0, rect, diag
        lens = np.array([len(r) for r in rows], dtype=np.int64)
        self.rp = np.zeros(self.nrows + 1, dtype=np.int32)
        self.rp[1:] = np.cumsum(lens)
        self.ci = (np.concatenate(rows) if lens.sum() else np.zeros(0)).astype(np.int32)
        self.va = (np.concatenate(vals) if lens.sum() else np.zeros(0)).astype(np.float64)
        assert np.array_equal(self.va.astype(np.float32).astype(np.float64), self.va)        # both types see the same matrix
        self.x0 = 0 if rect else row0
        self.xlen = xlen if rect else self.nrows
        self.nglobal = nglobal if nglobal is not None else max(row0 + self.nrows, self.x0 + self.xlen)
        self.lens, self.rowid = lens, np.repeat(np.arange(self.nrows), lens)
        l = self.ci.astype(np.int64) - self.x0
        self.halo_lo = int(max(0, -(l.min(initial=0))))
        self.halo_hi = int(max(0, l.max(initial=0) - self.xlen + 1))

    def values(self, dt):
        return np.ascontiguousarray(self.va.astype(NPDT[dt]))


def _pick(rng, k):
    return rng.choice(VALSET, size=k, replace=False) * rng.choice([-1.0, 1.0], size=k)


def _offset_rows(nglobal, r0, r1, table_of, wrap=False):
    """rows [r0, r1) of the operator whose row g has the entries table_of(g) = [(offset, value)] (columns outside the operator
    are dropped, or wrapped around); columns ascending, as a CSR matrix has them"""
    rows, vals = [], []
    for g in range(r0, r1):
        ent = []
        for off, v in table_of(g):
            j = g + off
            if wrap:
                j %= nglobal
            if 0 <= j < nglobal:
                ent.append((j, v))
        ent.sort()
        assert len({j for j, _ in ent}) == len(ent)
        rows.append(np.array([j for j, _ in ent], dtype=np.int64))
        vals.append(np.array([v for _, v in ent], dtype=np.float64))
    return rows, vals


def _lattice_table(L, seed):
    rng = np.random.default_rng(seed)
    offs = list(range(-(L // 2), L - L // 2))
    base = _pick(rng, L)
    other = base.copy()
    other[offs.index(0)] = _pick(rng, 1)[0] * 1.5                 # the two site types differ on the diagonal and in the last entry
    other[-1] = -base[-1] * 0.5
    tabs = [list(zip(offs, base)), list(zip(offs, other))]
    return lambda g: tabs[(g // 5) % 2]


def _grid_table(dims, seed):
    rng = np.random.default_rng(seed)
    nd = len(dims)
    v = _pick(rng, 2 * nd + 1)
    strides = [int(np.prod(dims[:d])) for d in range(nd)]

    def table(g):
        ent = [(0, v[0])]
        for d in range(nd):
            i = (g // strides[d]) % dims[d]
            if i > 0:
                ent.append((-strides[d], v[1 + 2 * d]))
            if i < dims[d] - 1:
                ent.append((strides[d], v[2 + 2 * d]))
        return ent
    return table


def _operator(op):
    """(nglobal, table_of, wrap) of a named global operator"""
    kind, _, arg = op.partition("@")
    if kind == "lap1d":
        n = int(arg)
        return n, (lambda g: [(-1, -0.75), (0, 2.5), (1, -1.25)]), False
    if kind == "lattice":
        L, _, n = arg.partition("/")
        return int(n or 1537), _lattice_table(int(L), 300 + int(L)), False
    if kind == "ring":
        tabs = [[(-1, -1.5), (0, 3.0), (1, -0.25)], [(-1, -1.5), (0, 0.375), (1, 2.0)]]
        return int(arg), (lambda g: tabs[(g // 5) % 2]), True
    if kind in ("lap2d", "lap3d"):
        dims = tuple(int(s) for s in arg.split("x"))
        return int(np.prod(dims)), _grid_table(dims, 400 + len(dims) + dims[0]), False
    raise ValueError(op)


@functools.lru_cache(maxsize=None)
def matrix(name):
    if name.startswith("diag:"):
        rest = name[5:]
        nodiag = rest.startswith("nodiag:")
        B = matrix(rest[7:] if nodiag else rest)
        rng = np.random.default_rng(zlib.crc32(name.encode()))
        rows, vals = [], []
        for i in range(B.nrows):
            c, v = B.ci[B.rp[i]:B.rp[i + 1]].astype(np.int64), B.va[B.rp[i]:B.rp[i + 1]].copy()
            d = c == B.row0 + i
            if nodiag and i % 11 == 3:
                c, v = c[~d], v[~d]
            else:
                v[d] = np.float32(rng.standard_normal() * 10.0 ** rng.uniform(-1.0, 1.0))
            rows.append(c)
            vals.append(v)
        return Mat(name, rows, vals, row0=B.row0, nglobal=B.nglobal, diag=True)
    if name.startswith("slab:"):
        _, op, row0, m = name.split(":")
        n, table, wrap = _operator(op)
        rows, vals = _offset_rows(n, int(row0), int(row0) + int(m), table, wrap)
        return Mat(name, rows, vals, row0=int(row0), nglobal=n)
    if name == "holes":
        n, table, _ = _operator("lattice@3/1100")
        rows, vals = _offset_rows(n, 0, n, lambda g: [] if g % 7 == 3 else table(g))
        return Mat(name, rows, vals)
    if name in ("npat256", "npat257"):
        k, n = int(name[4:]), 600
        v = (np.arange(n) % k + 1) / 32.0                       # k distinct values, exact in float
        return Mat(name, [np.array([i]) for i in range(n)], [np.array([x]) for x in v])
    if name == "row9":
        n, table, _ = _operator("lap1d@64")
        nine = [(o, 0.5 + 0.125 * o) for o in range(-4, 5)]
        rows, vals = _offset_rows(n, 0, n, lambda g: nine if g == 20 else table(g))
        return Mat(name, rows, vals)
    if name.startswith("pb_"):
        return _pb_matrix(name)
    n, table, wrap = _operator(name)
    rows, vals = _offset_rows(n, 0, n, table, wrap)
    return Mat(name, rows, vals)


LAP1D = [1, 2, 511, 512, 513, 1024, 3584, 4096, 4097, 6144, 10240]
LOCAL = [f"lap1d@{n}" for n in LAP1D] + [f"lattice@{L}" for L in range(1, 9)] + ["ring@2048", "lap2d@32x64", "lap2d@37x41", "lap3d@8x8x40", "holes", "npat256"]
DECLINED = ["npat257", "row9"]
SLABS = ["slab:lattice@8/4000:1000:1536",         # chunk 0 guarded (r0 + minoff < 0), chunk 1 inner, chunk 2 guarded (maxoff)
         "slab:lattice@2/4000:1000:1536", "slab:lattice@4/4000:1000:1536", "slab:lattice@6/4000:1000:1536",
         "slab:lattice@8/4000:3700:300",          # halo only below, m < 512: every row through the guard path
         "slab:lattice@8/4000:0:700",             # halo only above
         "slab:lattice@8/4000:2:600",             # row0 = 2 smaller than the reach 4: the halo is shorter than the reach
         "slab:ring@3000:0:1100",                 # the wrap-around entry of row 0 lies 1900 entries above the slab
         "slab:ring@3000:1000:1536",
         "slab:lap2d@32x64:20:1100",              # row0 = 20 smaller than the reach 32
         "slab:lap2d@37x41:500:400",              # m < 512, halo on both sides
         "slab:lap3d@8x8x40:640:1536"]
TWINS = [f"diag:lattice@{L}" for L in range(1, 9)] + ["diag:lap2d@37x41", "diag:nodiag:lattice@4", "diag:nodiag:holes"] + \
        [f"diag:slab:lattice@{L}/4000:1000:1536" for L in (2, 4, 6, 8)] + ["diag:slab:lattice@8/4000:3700:300"]
PAT_MATS = LOCAL + SLABS + TWINS


# ------------------------------------------------------------------------------------------------------------------
# the row-pattern form, restated from csrc/hipk_sparse_pat.hip
# ------------------------------------------------------------------------------------------------------------------
class PatInfo:
    pass


def pat_width(maxlen):
    return 3 if maxlen <= 3 else 5 if maxlen <= 5 else 7 if maxlen <= 7 else 8


@functools.lru_cache(maxsize=None)
def pat_info(name):
    """hipk_pat_build, and hipk_pat_build_diag for a twin whose exact scan gives up: None when the matrix is declined"""
    M = matrix(name)
    if M.rect or M.nrows == 0 or M.lens.max(initial=0) > PAT_MAXLEN:
        return None

    def scan(split):
        index, pid, pats = {}, np.zeros(M.nrows, dtype=np.int64), []
        for i in range(M.nrows):
            off = tuple(int(c) - (M.row0 + i) for c in M.ci[M.rp[i]:M.rp[i + 1]])
            val = tuple(M.va[M.rp[i]:M.rp[i + 1]])
            ds = -1
            if split and 0 in off:
                ds = off.index(0)
                val = val[:ds] + (0.0,) + val[ds + 1:]
            key = (off, val, ds)
            if key not in index:
                if len(pats) >= PAT_MAXPAT:
                    return None
                index[key] = len(pats)
                pats.append(key)
            pid[i] = index[key]
        return pid, pats

    got, split = scan(False), False
    if got is None and M.diag:
        got, split = scan(True), True
    if got is None:
        return None
    I = PatInfo()
    I.pid, I.pats = got
    I.diag, I.npat = split, len(I.pats)
    I.plen = np.array([len(p[0]) for p in I.pats])
    I.ml = pat_width(int(I.plen.max()))
    offs = [o for p in I.pats for o in p[0]]
    I.minoff, I.maxoff = min(offs + [0]), max(offs + [0])
    I.ds = np.array([p[2] for p in I.pats])
    I.nch = -(-M.nrows // CHUNK)
    I.halo = M.halo_lo > 0 or M.halo_hi > 0
    return I


def grid_of(nch, resident=1 << 20):
    """hipk_pat_grid_kind: the resident set (at least 1024 workgroups on this part) never binds at these sizes"""
    g = min(resident, nch) // 8 * 8
    return max(8, g)


def product_bytes_of(name, dt, fused):
    M, I = matrix(name), pat_info(name)
    es = np.dtype(NPDT[dt]).itemsize
    return float(M.nrows) * (1.0 + ((3.0 if fused else 2.0) + (1.0 if I.diag else 0.0)) * es)


def branch_of(c):
    """the instantiations of pat_kernel a case launches (type, table width, kind, local | halo, exact | diag); the row tiles for
    a declined matrix and for more than one column; nothing for a call that is declined before any launch"""
    if c.get("rc"):
        return []
    I, t = pat_info(c["mat"]), TNAME[c["dt"]]
    if I is None or (c["ep"] == "matvec" and c["w"] != 1):
        return [("row tiles", t)]
    kind = {"matvec": "plain", "scaled": "fused", "tail": "fused", "cheb": "cheb"}[c["ep"]]
    return [("pat_kernel", t, I.ml, kind, "halo" if I.halo else "local", "diag" if I.diag else "exact")]


@functools.lru_cache(maxsize=None)
def cells_of_matrix(name):
    """the per-chunk paths of pat_kernel's loop on this matrix: cells (path, axis, value) and launch-level marks"""
    M, I = matrix(name), pat_info(name)
    cells, marks = set(), set()
    if I is None:
        return cells, marks
    n, last = M.nrows, M.nrows - 1
    for c in range(I.nch):
        r0 = c * CHUNK
        inner = r0 + CHUNK <= n and (not I.halo or (r0 + I.minoff >= 0 and r0 + CHUNK - 1 + I.maxoff < n))
        path = "inner" if inner else "guard"
        near = r0 + CHUNK + I.maxoff >= n
        rows = np.arange(r0, min(r0 + CHUNK, n))
        for a in range(r0, min(r0 + CHUNK, n), 2):
            if a + 1 > last:
                cells.add((path, "single", True))
                continue
            cells.add((path, "single", False))
            same = I.pid[a] == I.pid[a + 1]
            cells.add((path, "pair", "same" if same else ("split+near" if (inner and near) else "split")))
        cells.add((path, "clamped", r0 + CHUNK > n))
        if r0 + CHUNK > n:
            cells.add((path, "clamped", False))                       # the rows that exist in a ragged chunk
        for v in set((I.plen[I.pid[rows]] < I.ml).tolist()):
            cells.add((path, "padded", v))
        if len(M.ci):
            sel = (M.rowid >= r0) & (M.rowid < r0 + CHUNK)
            l = M.ci[sel].astype(np.int64) - M.x0
            for nm, hit in (("lo", l < 0), ("own", (l >= 0) & (l < n)), ("hi", l >= n)):
                if hit.any():
                    cells.add((path, "source", nm))
        if (I.plen[I.pid[rows]] < I.ml).any() or (I.plen[I.pid[rows]] == 0).any():
            cells.add((path, "source", "own"))                        # a padded entry gathers the row's own x
        marks.add(("base below x", inner and r0 + I.minoff < 0))
    gx = grid_of(I.nch)
    per, J = -(-I.nch // 8), gx >> 3
    for q in range(8):
        c_lo, c_hi = q * per, min(q * per + per, I.nch)
        marks.add(("idle XCD", c_lo >= c_hi))
        for j in range(J):
            trips = len(range(c_lo + j, c_hi, J))
            if trips:
                marks.add(("trips", trips))
    marks |= {("nch", I.nch), ("J", J), ("npat", I.npat)}
    if I.diag:
        marks |= {("dslot", int(d)) for d in I.ds}
    return cells, marks


PATHS = ("inner", "guard")
AXES = {"pair": ("same", "split", "split+near"), "clamped": (True, False), "single": (True, False), "source": ("own", "lo", "hi"),
        "padded": (True, False)}
UNREACHABLE = {
    ("inner", "source", "lo"): "an inner chunk lies inside the slab together with every entry its rows reference: no halo source",
    ("inner", "source", "hi"): "an inner chunk lies inside the slab together with every entry its rows reference: no halo source",
    ("inner", "clamped", True): "an inner chunk is a full chunk: r0 + 512 <= nrows, no row is clamped",
    ("inner", "single", True): "an inner chunk is a full chunk of 256 whole pairs",
    ("guard", "pair", "split+near"): "`near` is computed and read by the buffer-addressed form only; the guard path loads row by row",
}
REACHABLE = {(p, a, v) for p in PATHS for a, vs in AXES.items() for v in vs} - set(UNREACHABLE)
WANTED_MARKS = ({("trips", 1), ("trips", 2), ("idle XCD", True), ("idle XCD", False), ("J", 1), ("J", 2), ("base below x", True), ("base below x", False),
                 ("npat", 1), ("npat", 256), ("dslot", -1), ("dslot", 0), ("dslot", 4)} | {("nch", k) for k in (1, 2, 7, 8, 9, 12, 20)})


def wanted_instantiations():
    want = {("pat_kernel", t, ml, k, h, d) for t in ("f64", "f32") for ml in (3, 5, 7, 8) for k in ("plain", "fused") for h in ("local", "halo")
            for d in ("exact", "diag")}
    want |= {("pat_kernel", t, ml, "cheb", "local", d) for t in ("f64", "f32") for ml in (3, 5, 7, 8) for d in ("exact", "diag")}
    return want


# ------------------------------------------------------------------------------------------------------------------
# the panel-blocked form, restated from hipk_pb_build (csrc/hipk_sparse_pb.hip)
# ------------------------------------------------------------------------------------------------------------------
PB_KNOBS = {
    "pb": dict(env={"HIPK_PB": "1", "HIPK_PB_KB": "8"}, U=4, tile=640),
    "pb_u2_tile1": dict(env={"HIPK_PB": "1", "HIPK_PB_KB": "8", "HIPK_PB_U": "2", "HIPK_PB_TILE": "1"}, U=2, tile=1),
    "pb_u8": dict(env={"HIPK_PB": "1", "HIPK_PB_KB": "8", "HIPK_PB_U": "8"}, U=8, tile=640),
}
PB_MATS = ["pb_wide", "pb_tall", "pb_seg"]


def _pb_matrix(name):
    rng = np.random.default_rng(zlib.crc32(name.encode()))
    if name == "pb_wide":                 # 700 x 5000, 8 scattered entries per row; row 5 has 300 entries inside the first panel
        rows = CB._scatter_rows([8] * 700, 5000, 51)
        rows[5] = np.sort(rng.choice(1024, size=300, replace=False))
        m, n = 700, 5000
    elif name == "pb_tall":               # 6000 x 300, most rows empty: one panel, tiles of 2048 rows
        rows = CB._scatter_rows(rng.integers(0, 2, size=6000) * rng.integers(0, 2, size=6000), 300, 52)
        m, n = 6000, 300
    elif name == "pb_seg":
        # 256 x 4096; columns [0, 1024): 512, 507, 5, 0 entries in the rows [0, 64), [64, 128), [128, 192), [192, 256) (1024 in all);
        # [1024, 2048): none; [2048, 3072): 40 in the rows [128, 192); [3072, 4096): 612 in the rows [192, 256)
        m, n, rows = 256, 4096, [[] for _ in range(256)]

        def put(r0, total, c0):
            per = [total // 64 + (1 if i < total % 64 else 0) for i in range(64)]
            for i, k in enumerate(per):
                rows[r0 + i] += list(c0 + np.sort(rng.choice(1024, size=k, replace=False)))
        put(0, 512, 0); put(64, 507, 0); put(128, 5, 0); put(128, 40, 2048); put(192, 612, 3072)
        rows = [np.array(sorted(r), dtype=np.int64) for r in rows]
    else:
        raise ValueError(name)
    vals = [rng.choice(VALSET, size=len(r)) * rng.choice([-1.0, 1.0], size=len(r)) for r in rows]
    return Mat(name, rows, vals, rect=True, xlen=n)


@functools.lru_cache(maxsize=None)
def pb_plan(name, dt, knobs):
    """(cb, P, RT, ntiles, seg) with seg[tile, panel] the entries of a (tile, panel) segment"""
    M, K = matrix(name), PB_KNOBS[knobs]
    es, m, n, nnz = np.dtype(NPDT[dt]).itemsize, M.nrows, M.xlen, len(M.ci)
    cb = 10
    while (1 << cb) * es < 8 * 1024:
        cb += 1
    W = 1 << cb
    Pn = -(-n // W)
    assert Pn <= 256
    per = nnz / m / Pn
    RT = 64
    while RT < 2048 and RT < (1 << (32 - cb)) // 2 and RT * per < K["tile"]:
        RT *= 2
    ntiles = -(-m // RT)
    seg = np.zeros((ntiles, Pn), dtype=np.int64)
    np.add.at(seg, (M.rowid // RT, M.ci.astype(np.int64) >> cb), 1)
    return cb, Pn, RT, ntiles, seg


def pb_cells(name, dt, knobs):
    cb, Pn, RT, ntiles, seg = pb_plan(name, dt, knobs)
    M, U = matrix(name), PB_KNOBS[knobs]["U"]
    step = 64 * U
    cells = {("inst", TNAME[dt], U), ("P", "1" if Pn == 1 else ">1"), ("RT", RT), ("ntiles%4", ntiles % 4 != 0), ("ragged tile", M.nrows % RT != 0)}
    if Pn > 1:
        cells.add(("partial last panel", M.xlen % (1 << cb) != 0))
    for s in seg.ravel():
        kind = "empty" if s == 0 else "1-63" if s < 64 else "multiple" if s % step == 0 else "multiple+rest" if s > step else "64..step-1"
        cells.add(("segment", kind))
    inpanel = np.zeros((M.nrows, Pn), dtype=np.int64)
    np.add.at(inpanel, (M.rowid, M.ci.astype(np.int64) >> cb), 1)
    if inpanel.max(initial=0) >= 300:
        cells.add(("row of 300 in one panel", True))
    return cells


PB_WANTED = ({("inst", t, u) for t in ("f64", "f32") for u in (2, 4, 8)} | {("P", "1"), ("P", ">1"), ("partial last panel", True), ("RT", 64), ("RT", 2048),
             ("ntiles%4", True), ("ragged tile", True), ("row of 300 in one panel", True)} |
             {("segment", k) for k in ("empty", "1-63", "multiple", "multiple+rest")})


# ------------------------------------------------------------------------------------------------------------------
# the stencil
# ------------------------------------------------------------------------------------------------------------------
def _grid3(g):
    return tuple(g) + (0,) * (3 - len(g))            # ny / nz passed as 0 must behave as 1


STENCIL = []                                         # (grid, row0, m): whole and in slabs
for _g, _slabs in (((1000,), [(0, 1000), (0, 400), (400, 600), (300, 333)]),
                   ((7, 5), [(0, 35), (0, 14), (21, 14), (10, 13), (3, 20), (16, 4)]),           # row0 = 3 < 7: halo shorter than the reach; 4 rows: thinner than a line
                   ((5, 4, 3), [(0, 60), (0, 20), (40, 20), (20, 20), (7, 40), (25, 9)]),        # row0 = 7 < 20; 9 rows: thinner than a plane
                   ((1, 6), [(0, 6), (0, 2), (4, 2), (2, 3)]),
                   ((1, 1, 1), [(0, 1)])):
    STENCIL += [(_g, r0, m) for r0, m in _slabs]


@functools.lru_cache(maxsize=None)
def stencil_matrix(grid, row0, m):
    """the header's definition: diagonal 2 dims, -1 to each grid neighbour, Dirichlet; dims = 3 with nz > 1, 2 with ny > 1, else 1"""
    g3 = tuple(max(1, v) for v in _grid3(grid))
    dims = 3 if g3[2] > 1 else 2 if g3[1] > 1 else 1
    n = g3[0] * g3[1] * g3[2]
    strides = (1, g3[0], g3[0] * g3[1])

    def table(g):
        ent = [(0, 2.0 * dims)]
        for d in range(3):
            i = (g // strides[d]) % g3[d]
            ent += [(-strides[d], -1.0)] * (i > 0) + [(strides[d], -1.0)] * (i < g3[d] - 1)
        return ent
    rows, vals = _offset_rows(n, row0, row0 + m, table)
    M = Mat(f"stencil{grid}:{row0}:{m}", rows, vals, row0=row0, nglobal=n)
    reach = strides[dims - 1] if dims > 1 else 1
    M.halo_lo, M.halo_hi = min(reach, row0), min(reach, n - row0 - m)          # hipk_stencil_create: the reach, cut at the operator's ends
    M.grid3, M.dims = _grid3(grid), dims
    return M


# ------------------------------------------------------------------------------------------------------------------
# case tables (static)
# ------------------------------------------------------------------------------------------------------------------
SCALED_MATS = ["lap1d@1", "lap1d@513", "lap1d@4097", "lap1d@10240", "lattice@2", "lattice@4", "lattice@6", "lattice@8", "ring@2048", "lap2d@37x41",
               "lap3d@8x8x40", "holes", "npat256", "npat257"] + SLABS[:5] + ["slab:ring@3000:0:1100", "slab:lap2d@37x41:500:400"] + \
              ["diag:lattice@2", "diag:lattice@4", "diag:lattice@6", "diag:lattice@8", "diag:nodiag:lattice@4"] + TWINS[-5:]
TAIL_MATS = ["lattice@8", "lap2d@37x41", "diag:lattice@8", "diag:lap2d@37x41"]
CHEB_MATS = ["lap1d@513", "lap1d@4097", "lattice@2", "lattice@4", "lattice@6", "lattice@8", "ring@2048", "lap2d@32x64", "holes",
             "diag:lattice@2", "diag:lattice@4", "diag:lattice@6", "diag:lattice@8", "diag:nodiag:lattice@4", "diag:lap2d@37x41"]
CHEB_VARIANTS = [(1, None), (3, "given"), (8, "alias")]
CHEB_ALL9 = "lattice@8"
STENCIL_WIDTHS = [1, 3, 8]
PB_WIDTHS = {"pb_wide": [1, 2, 3], "pb_tall": [1, 2], "pb_seg": [1]}


def _cases():
    out = []
    for dt in RTYPES:
        for fl in FLAVOURS:
            out += [dict(ep="matvec", dt=dt, mat=m, w=1, flavour=fl) for m in PAT_MATS + DECLINED]
            out.append(dict(ep="matvec", dt=dt, mat="lattice@8", w=2, flavour=fl))              # two columns: routed to the row tiles
            out += [dict(ep="scaled", dt=dt, mat=m, w=1, flavour=fl, norm2=n2, fin=fin) for m in SCALED_MATS for n2 in (True, False) for fin in (0, 4)]
            out.append(dict(ep="scaled", dt=dt, mat="lattice@3", w=1, flavour=fl, norm2=True, fin=0, rc=-1, alias=True))
            out += [dict(ep="tail", dt=dt, mat=m, w=1, flavour=fl) for m in TAIL_MATS]
            for i, m in enumerate(CHEB_MATS):
                vs = [(nx, yp) for nx in (1, 3, 8) for yp in (None, "given", "alias")] if m == CHEB_ALL9 else [CHEB_VARIANTS[(i + k) % 3] for k in range(2)] + \
                     [(CHEB_VARIANTS[(i + 2) % 3][0], CHEB_VARIANTS[i % 3][1])]
                out += [dict(ep="cheb", dt=dt, mat=m, w=nx, flavour=fl, yprev=yp) for nx, yp in vs]
            out += [dict(ep="cheb", dt=dt, mat="lattice@3", w=1, flavour=fl, yprev=None, rc=-1, outyk=True),
                    dict(ep="cheb", dt=dt, mat="lattice@3", w=9, flavour=fl, yprev=None, rc=-1),
                    dict(ep="cheb", dt=dt, mat=SLABS[0], w=1, flavour=fl, yprev=None, rc=1)]
            out += [dict(ep="stencil", dt=dt, grid=g, row0=r0, m=m, w=w, flavour=fl) for g, r0, m in STENCIL for w in STENCIL_WIDTHS]
    for dt in (F.HIPK_C64, F.HIPK_C32):
        out.append(dict(ep="stencil", dt=dt, grid=(7, 5), row0=0, m=35, w=1, flavour="even", rc=-44))
    for kn in PB_KNOBS:
        for di, dt in enumerate(RTYPES):
            out += [dict(ep="pb", dt=dt, mat=m, w=w, flavour=FLAVOURS[(i + j + di) % 2], knobs=kn)
                    for i, m in enumerate(PB_MATS) for j, w in enumerate(PB_WIDTHS[m])]
    return out


CASES = _cases()

ORACLE_SAME = {
    "scaled/fin": "hipk_set_inkernel_fin exists only in the device library; the oracle has one second stage, so both settings run the same loop",
    "matvec/format": "hipk_set_spmv_format, hipk_csr_create_opts and the form queries exist only in the device library; the oracle has one CSR loop",
    "cheb": "the oracle has no hipk_csr_cheb_step: its product followed by the combination in numpy double takes its place, and the "
            "return codes of the declined calls are checked on the device only",
    "tail": "hipk_tail_defer of the oracle accepts nothing: the same calls run as the sequence of separate second stages",
    "pb": "the HIPK_PB* knobs select the device form; the oracle has one loop (hipk_csr_create_rect)",
}


def case_id(c):
    keys = [k for k in ("w", "norm2", "fin", "yprev", "rc", "alias", "outyk", "knobs", "flavour") if k in c]
    what = c["mat"] if "mat" in c else f"{c['grid']}:{c['row0']}:{c['m']}"
    return f"{c['ep']}[{TNAME[c['dt']]},{what}," + ",".join(f"{k}={c[k]}" for k in keys) + "]"


def groups(knobs=False):
    """[(id, cases)]: one test per (entry point, type, flavour); with knobs=True per (knob set, type)"""
    out = {}
    for c in CASES:
        if bool(c.get("knobs")) != knobs:
            continue
        key = f"{c['knobs']}-{TNAME[c['dt']]}" if knobs else f"{c['ep']}-{TNAME[c['dt']]}-{c['flavour']}"
        out.setdefault(key, []).append(c)
    return sorted(out.items())


# ------------------------------------------------------------------------------------------------------------------
# runners
# ------------------------------------------------------------------------------------------------------------------
def _rand(rng, shape, dt):
    return (rng.standard_normal(shape) * np.linspace(1.0, 3.0, shape[0])[:, None]).astype(NPDT[dt])


@functools.lru_cache(maxsize=None)
def _inputs(ep, dt, key, w, ref=True):
    """the data of a case and its reference: the same for both flavours and both sides, computed once, never changed"""
    M = stencil_matrix(*key) if ep == "stencil" else matrix(key)
    rng = np.random.default_rng(zlib.crc32(f"{ep},{dt},{key},{w}".encode()))
    X, lo, hi = _rand(rng, (w, M.xlen), dt), _rand(rng, (w, M.halo_lo), dt), _rand(rng, (w, M.halo_hi), dt)
    norm2 = float(rng.uniform(0.5, 9.0))
    r = CB.ref_matvec(M, M, dt, X, lo, hi) if ref else None
    for a in (X, lo, hi):
        a.setflags(write=False)
    return X, lo, hi, norm2, r


def _vp(a):
    return a.ctypes.data_as(C.c_void_p)


def _declare(lib):
    for name in ("hipk_csr_panels", "hipk_csr_format", "hipk_csr_npatterns", "hipk_csr_pattern_diag"):
        if hasattr(lib, name):
            getattr(lib, name).argtypes, getattr(lib, name).restype = [C.c_void_p], C.c_int
    if hasattr(lib, "hipk_set_inkernel_fin"):
        lib.hipk_set_inkernel_fin.argtypes, lib.hipk_set_inkernel_fin.restype = [C.c_int], C.c_int
    if hasattr(lib, "hipk_tail_abandon"):
        lib.hipk_tail_abandon.argtypes, lib.hipk_tail_abandon.restype = [C.c_void_p], None


def _create(side, c, M):
    """the operator; on the device: in the form pat_info / pb_plan say, with the bytes and halo extents the restatement gives"""
    dt, cid, A, va = c["dt"], case_id(c), C.c_void_p(), M.values(c["dt"])
    _declare(side.lib)
    dev = side.name == "hip" and hasattr(side.lib, "hipk_csr_format")
    if M.rect:
        rc = side.lib.hipk_csr_create_rect(side.ctx, dt, M.nrows, M.xlen, _vp(M.rp), _vp(M.ci), _vp(va), C.byref(A))
    elif M.diag and dev:
        rc = side.lib.hipk_csr_create_opts(side.ctx, dt, M.nrows, M.nglobal, M.row0, _vp(M.rp), _vp(M.ci), _vp(va), DIAG_PATTERNS, C.byref(A))
    else:
        rc = side.lib.hipk_csr_create(side.ctx, dt, M.nrows, M.nglobal, M.row0, _vp(M.rp), _vp(M.ci), _vp(va), C.byref(A))
    assert rc == 0 and A, f"{cid}: create rc = {rc}"
    assert (side.lib.hipk_csr_halo_lo(A), side.lib.hipk_csr_halo_hi(A)) == (M.halo_lo, M.halo_hi), cid
    if dev:
        lib = side.lib
        form = (lib.hipk_csr_format(A), lib.hipk_csr_npatterns(A), lib.hipk_csr_pattern_diag(A), lib.hipk_csr_panels(A))
        if c["ep"] == "pb":
            assert form == (1, 0, 0, pb_plan(c["mat"], dt, c["knobs"])[1]), f"{cid}: (format, patterns, diag, panels) = {form}"
        else:
            I = pat_info(c["mat"])
            want = (0, 0, 0, 0) if I is None else (2, I.npat, int(I.diag), 0)
            assert form == want, f"{cid}: (format, patterns, diag, panels) = {form}, restated {want}"
            if I is not None:
                got = tuple(lib.hipk_csr_product_bytes(A, f) for f in (0, 1))
                assert got == tuple(product_bytes_of(c["mat"], dt, f) for f in (0, 1)), (cid, got)
    return A


def _run_matvec(side, c, rep):
    """hipk_csr_matvec twice, and (one column, device) once more on the row tiles after hipk_set_spmv_format(0): bit-identical"""
    dt, w, cid, npdt = c["dt"], c["w"], case_id(c), np.dtype(NPDT[c["dt"]])
    M = matrix(c["mat"])
    X, lo, hi, _, (yr, S, n) = _inputs("matvec" if c["ep"] == "pb" else c["ep"], dt, c["mat"], w)
    sh = 1 if c["flavour"] == "odd" else 0
    ldx, ldy, ld_lo, ld_hi = _lds(c["flavour"], [M.xlen, M.nrows, M.halo_lo, M.halo_hi])
    tiles_too = side.name == "hip" and hasattr(side.lib, "hipk_set_spmv_format") and w == 1 and c["ep"] == "matvec"
    xo = Operand(npdt, M.xlen, w, ldx, sh)
    xo.fill(range(w), X)
    ys = [Operand(npdt, M.nrows, w, ldy, sh) for _ in range(3 if tiles_too else 2)]
    for y in ys:
        y.expect(range(w))
    A = _create(side, c, M)
    try:
        tx, tys = side.arr(xo.host), [side.arr(y.host) for y in ys]
        halos = CB._halo_ops(side, c, M, npdt, lo, hi, ld_lo, ld_hi, w)
        CB._set_halo(side, A, halos)
        for k, (y, ty) in enumerate(zip(ys, tys)):
            old = side.lib.hipk_set_spmv_format(0) if k == 2 else None
            try:
                if k == 2:
                    assert side.lib.hipk_csr_format(A) == 0, cid
                rc = side.lib.hipk_csr_matvec(A, None, xo.base(side, tx), xo.ld, y.base(side, ty), y.ld, w)
            finally:
                if k == 2:
                    side.lib.hipk_set_spmv_format(old)
            assert rc == 0, f"{cid}: rc = {rc}"
        named = [("x", xo, tx)] + [(f"y (call {k + 1})", y, ty) for k, (y, ty) in enumerate(zip(ys, tys))]
        named += [(nm, op, t) for nm, (op, t) in zip(("halo lo", "halo hi"), halos) if op is not None]
        got = P._finish(side, rep, cid, named)
    finally:
        side.lib.hipk_csr_destroy(A)
    rep.same_bits(f"{cid} y: the same product issued twice", got[1], got[2])
    if tiles_too:
        rep.same_bits(f"{cid} y: the form against the row tiles (hipk_set_spmv_format(0))", got[1], got[3])
    CB._cmp_rows(rep, f"{cid} y", dt, ys[0].take(got[1], range(w)), yr, S, n[None, :])


def _run_scaled(side, c, rep):
    dt, cid, npdt = c["dt"], case_id(c), np.dtype(NPDT[c["dt"]])
    M = matrix(c["mat"])
    X, lo, hi, norm2, _ = _inputs("scaled", dt, c["mat"], 1, False)
    want_rc, m = c.get("rc", 0), M.nrows
    sh = 1 if c["flavour"] == "odd" else 0
    ldx, ldo, ldy, ld_lo, ld_hi = _lds(c["flavour"], [m, m, m, M.halo_lo, M.halo_hi])
    xo = Operand(npdt, m, 1, ldx, sh)
    xo.fill(0, X)
    n2 = small(1)
    n2.fill(0, [norm2])
    outs = [(Operand(npdt, m, 1, ldo, sh), Operand(npdt, m, 1, ldy, sh), small(1)) for _ in range(2)]
    if want_rc == 0:
        for o in outs:
            for op in o:
                op.expect(0)
    A = _create(side, c, M)
    switch = hasattr(side.lib, "hipk_set_inkernel_fin")          # ORACLE_SAME["scaled/fin"]
    old = side.lib.hipk_set_inkernel_fin(c["fin"]) if switch else None
    try:
        tx, tn = side.arr(xo.host), side.arr(n2.host)
        touts = [tuple(side.arr(op.host) for op in o) for o in outs]
        halos = CB._halo_ops(side, c, M, npdt, lo, hi, ld_lo, ld_hi, 1)
        CB._set_halo(side, A, halos)
        for (xout, y, dot), (txo, ty, td) in zip(outs, touts):
            rc = side.lib.hipk_csr_matvec_scaled(A, side.ctx, xo.base(side, tx), n2.base(side, tn) if c["norm2"] else None,
                                                 xo.base(side, tx) if c.get("alias") else xout.base(side, txo), y.base(side, ty), dot.base(side, td))
            assert rc == want_rc, f"{cid}: rc = {rc}, the header says {want_rc}"
        named = [("x", xo, tx), ("norm2", n2, tn)]
        for i, (o, to) in enumerate(zip(outs, touts)):
            named += [(f"{nm} (call {i + 1})", op, t) for nm, op, t in zip(("xout", "y", "dot"), o, to)]
        named += [(nm, op, t) for nm, (op, t) in zip(("halo lo", "halo hi"), halos) if op is not None]
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
    _check_scaled(rep, cid, M, dt, X[0], lo, hi, norm2 if c["norm2"] else None, xs, yst, dst)


def _check_scaled(rep, cid, M, dt, x, lo, hi, norm2, xs, yst, dst):
    ax, yr, S, Sh = CB.ref_scaled(M, M, dt, x, lo, hi, norm2, xs)
    rep.cmp(f"{cid} xout", xs, ax, bound_elem(dt, 1, np.abs(ax)))
    CB._cmp_rows(rep, f"{cid} y", dt, yst, yr, S, M.lens.astype(np.float64), extra=(2.0 * UNIT[dt] + 4.0 * U64) * Sh)
    xl, yl = np.asarray(xs, LD), np.asarray(yst, LD)
    rep.cmp(f"{cid} dot", dst, (xl * yl).sum(), bound_red(M.nrows, (np.abs(xl) * np.abs(yl)).sum(), dt, int(M.lens.max(initial=0)) + 2))


def _run_tail(side, c, rep):
    """hipk_tail_defer(ctx, 3), a one-column hipk_panel_project_to, the fused product, hipk_tail_finish"""
    dt, cid, npdt = c["dt"], case_id(c), np.dtype(NPDT[c["dt"]])
    M = matrix(c["mat"])
    m, k = M.nrows, 3
    rng = np.random.default_rng(zlib.crc32(f"tail,{dt},{c['mat']}".encode()))
    Vd, rd, cf = _rand(rng, (k, m), dt), _rand(rng, (1, m), dt), rng.standard_normal(k) * 0.3
    sh = 1 if c["flavour"] == "odd" else 0
    ldv, ldr, ldt, ldo, ldy = _lds(c["flavour"], [m, m, m, m, m])
    V, R, T, XO, Y = (Operand(npdt, m, nc, ld, sh) for nc, ld in ((k, ldv), (1, ldr), (1, ldt), (1, ldo), (1, ldy)))
    V.fill(range(k), Vd); R.fill(0, rd)
    coef, res = small(k), small(2)                              # res = [|t|^2, t'At]
    coef.fill(0, cf)
    for op in (T, XO, Y, res):
        op.expect(0)
    A = _create(side, c, M)
    try:
        tv, tr, tt, to, ty, tc, ts = (side.arr(op.host) for op in (V, R, T, XO, Y, coef, res))
        seg = (F.HipkSeg * 1)()
        seg[0].base, seg[0].ld, seg[0].ncols = V.base(side, tv).value, V.ld, k
        n2p, dotp = res.base(side, ts), side.ptr(ts, res.off + 1)
        acc = side.lib.hipk_tail_defer(side.ctx, 3)
        assert acc == (3 if side.name == "hip" and hasattr(side.lib, "hipk_csr_format") else 0), f"{cid}: hipk_tail_defer accepted {acc}"
        try:
            assert side.lib.hipk_panel_project_to(side.ctx, dt, m, seg, 1, coef.base(side, tc), coef.ld, R.base(side, tr), R.ld, T.base(side, tt), T.ld, 1, n2p) == 0, cid
            assert side.lib.hipk_tail_pending(side.ctx) == (1 if acc else 0), cid
            assert side.lib.hipk_csr_matvec_scaled(A, side.ctx, T.base(side, tt), n2p, XO.base(side, to), Y.base(side, ty), dotp) == 0, cid
            assert side.lib.hipk_tail_pending(side.ctx) == acc, cid
            assert side.lib.hipk_tail_finish(side.ctx, None, None, 0, dotp, None) == 0, cid
            assert side.lib.hipk_tail_pending(side.ctx) == 0, cid
        finally:
            side.lib.hipk_tail_abandon(side.ctx)
        got = P._finish(side, rep, cid, [("V", V, tv), ("r", R, tr), ("coef", coef, tc), ("t", T, tt), ("xout", XO, to), ("y", Y, ty), ("results", res, ts)])
    finally:
        side.lib.hipk_csr_destroy(A)
    t, xs, yst = T.take(got[3], 0)[0], XO.take(got[4], 0)[0], Y.take(got[5], 0)[0]
    n2, dot = float(got[6][res.off]), float(got[6][res.off + 1])
    tr_, St, n2r, Sn = P.ref_project(dt, Vd, cf[None, :], rd)
    rep.cmp(f"{cid} t", t, tr_[0], bound_elem(dt, k, St[0]))
    tl = np.asarray(t, LD)
    rep.cmp(f"{cid} |t|^2", n2, (tl * tl).sum(), bound_red(m, (tl * tl).sum()))
    a = 1.0 / np.sqrt(np.float64(n2))
    rep.same_bits(f"{cid} xout: scaled with the published |t|^2", xs, (a * t.astype(np.float64)).astype(npdt))
    empty = np.zeros((1, 0), npdt)
    _check_scaled(rep, cid, M, dt, t, empty, empty, n2, xs, yst, dot)


def _coef(w):
    cf = F.HipkChebCoef()
    k = min(w, 8)
    vals = dict(cy=np.linspace(0.625, -1.375, k), cp=np.linspace(-0.75, 0.5, k) - 0.0625, cx=np.linspace(1.5, 0.25, k), cw=np.linspace(-0.3125, 0.875, k))
    for nm, v in vals.items():
        for i in range(k):
            getattr(cf, nm)[i] = v[i]
    return cf, {nm: np.asarray(v, LD)[:, None] for nm, v in vals.items()}


def _run_cheb(side, c, rep):
    """Out = cy Yk + cp Yprev + cx X + cw (A Yk); on the oracle: its product and the combination in numpy double"""
    dt, w, cid, npdt = c["dt"], c["w"], case_id(c), np.dtype(NPDT[c["dt"]])
    M, want_rc, yp = matrix(c["mat"]), c.get("rc", 0), c["yprev"]
    dev = side.name == "hip" and hasattr(side.lib, "hipk_csr_format")
    if want_rc and not dev:
        return                                                    # ORACLE_SAME["cheb"]
    m = M.nrows
    wr = min(w, 8)
    Yk, _, _, _, ref = _inputs("cheb", dt, c["mat"], wr, not want_rc and not M.halo_lo and not M.halo_hi)
    rng = np.random.default_rng(zlib.crc32(f"cheb2,{dt},{c['mat']},{w}".encode()))
    Xd, Ypd = _rand(rng, (wr, m), dt), _rand(rng, (wr, m), dt)
    sh = 1 if c["flavour"] == "odd" else 0
    ldx, ldk, ldp, ldo = _lds(c["flavour"], [m, m, m, m])
    X, K_, Pv = Operand(npdt, m, wr, ldx, sh), Operand(npdt, m, wr, ldk, sh), Operand(npdt, m, wr, ldp, sh)
    X.fill(range(wr), Xd); K_.fill(range(wr), Yk); Pv.fill(range(wr), Ypd)
    outs = []
    for _ in range(2):
        if yp == "alias":
            o = Operand(npdt, m, wr, ldp, sh)
            o.fill(range(wr), Ypd)
        else:
            o = Operand(npdt, m, wr, ldo, sh)
        if not want_rc:
            o.expect(range(wr))
        outs.append(o)
    cf, cl = _coef(w)
    A = _create(side, dict(c, ep="cheb"), M)
    try:
        tx, tk, tp = side.arr(X.host), side.arr(K_.host), side.arr(Pv.host)
        touts = [side.arr(o.host) for o in outs]
        for o, to in zip(outs, touts):
            ypp, ypld = (None, 0) if yp is None else (o.base(side, to), o.ld) if yp == "alias" else (Pv.base(side, tp), Pv.ld)
            if dev:
                out_p = K_.base(side, tk) if c.get("outyk") else o.base(side, to)
                rc = side.lib.hipk_csr_cheb_step(A, None, w, C.byref(cf), X.base(side, tx), X.ld, K_.base(side, tk), K_.ld, ypp, ypld, out_p, o.ld)
                assert rc == want_rc, f"{cid}: rc = {rc}, the header says {want_rc}"
            else:
                tw = side.arr(np.full((wr, m), np.nan, npdt))
                assert side.lib.hipk_csr_matvec(A, None, K_.base(side, tk), K_.ld, side.ptr(tw), m, wr) == 0
                v = {nm: np.asarray(a, np.float64) for nm, a in cl.items()}
                comb = v["cx"] * Xd.astype(np.float64) + v["cy"] * Yk.astype(np.float64) + v["cw"] * tw.astype(np.float64)
                if yp is not None:
                    comb = comb + v["cp"] * Ypd.astype(np.float64)
                to[o.index(range(wr))] = comb.astype(npdt)
        got = P._finish(side, rep, cid, [("X", X, tx), ("Yk", K_, tk), ("Yprev", Pv, tp), ("Out (call 1)", outs[0], touts[0]), ("Out (call 2)", outs[1], touts[1])])
    finally:
        side.lib.hipk_csr_destroy(A)
    rep.same_bits(f"{cid} Out: the same step issued twice", got[3], got[4])
    if want_rc:
        return
    y, S, n = ref
    xl, kl, pl = np.asarray(Xd, LD), np.asarray(Yk, LD), np.asarray(Ypd, LD) * (0 if yp is None else 1)
    out = cl["cy"] * kl + cl["cp"] * pl + cl["cx"] * xl + cl["cw"] * y
    Sx = np.abs(cl["cy"] * kl) + np.abs(cl["cp"] * pl) + np.abs(cl["cx"] * xl) + np.abs(cl["cw"]) * S
    rep.cmp(f"{cid} Out", outs[0].take(got[3], range(wr)), out, bound_row(dt, n[None, :] + 3, Sx))


def _run_stencil(side, c, rep):
    dt, w, cid = c["dt"], c["w"], case_id(c)
    nx, ny, nz = _grid3(c["grid"])
    if c.get("rc"):
        A = C.c_void_p()
        rc = side.lib.hipk_stencil_create(side.ctx, dt, nx, ny, nz, c["row0"], c["m"], C.byref(A))
        if rc == 0:                                               # the header: complex types return -44 (at creation or at the product)
            z = side.arr(np.zeros(2 * c["m"] + 8, NPDT[dt]))
            rc = side.lib.hipk_csr_matvec(A, None, side.ptr(z), c["m"], side.ptr(z, c["m"] + 4), c["m"], 1)
            side.lib.hipk_csr_destroy(A)
        assert rc == c["rc"], f"{cid}: rc = {rc}, the header says {c['rc']}"
        return
    npdt = np.dtype(NPDT[dt])
    key = (c["grid"], c["row0"], c["m"])
    M = stencil_matrix(*key)
    X, lo, hi, _, (yr, S, n) = _inputs("stencil", dt, key, w)
    sh = 1 if c["flavour"] == "odd" else 0
    ldx, ldy, ld_lo, ld_hi = _lds(c["flavour"], [M.nrows, M.nrows, M.halo_lo, M.halo_hi])
    xo = Operand(npdt, M.nrows, w, ldx, sh)
    xo.fill(range(w), X)
    ys = [Operand(npdt, M.nrows, w, ldy, sh) for _ in range(2)]
    for y in ys:
        y.expect(range(w))
    A = C.c_void_p()
    assert side.lib.hipk_stencil_create(side.ctx, dt, nx, ny, nz, c["row0"], c["m"], C.byref(A)) == 0 and A, cid
    try:
        assert (side.lib.hipk_csr_halo_lo(A), side.lib.hipk_csr_halo_hi(A)) == (M.halo_lo, M.halo_hi), cid
        assert side.lib.hipk_csr_kind(A) == 1, cid
        _declare(side.lib)
        if side.name == "hip" and hasattr(side.lib, "hipk_csr_format"):
            assert side.lib.hipk_csr_format(A) == 3, cid
        tx, tys = side.arr(xo.host), [side.arr(y.host) for y in ys]
        halos = CB._halo_ops(side, c, M, npdt, lo, hi, ld_lo, ld_hi, w)
        CB._set_halo(side, A, halos)
        for y, ty in zip(ys, tys):
            assert side.lib.hipk_csr_matvec(A, None, xo.base(side, tx), xo.ld, y.base(side, ty), y.ld, w) == 0, cid
        named = [("x", xo, tx), ("y", ys[0], tys[0]), ("y (second call)", ys[1], tys[1])]
        named += [(nm, op, t) for nm, (op, t) in zip(("halo lo", "halo hi"), halos) if op is not None]
        got = P._finish(side, rep, cid, named)
    finally:
        side.lib.hipk_csr_destroy(A)
    rep.same_bits(f"{cid} y: the same product issued twice", got[1], got[2])
    CB._cmp_rows(rep, f"{cid} y", dt, ys[0].take(got[1], range(w)), yr, S, n[None, :])


RUNNERS = {"matvec": _run_matvec, "pb": _run_matvec, "scaled": _run_scaled, "tail": _run_tail, "cheb": _run_cheb, "stencil": _run_stencil}


def run_cases(side_factory, cases):
    return P.run_cases(side_factory, cases, RUNNERS)
