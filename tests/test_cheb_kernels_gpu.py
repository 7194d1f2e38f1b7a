"""The three device entry points of the Chebyshev preconditioner, shape by shape: hipk_csr_cheb_step (the fused step, an
epilogue of the row-pattern kernel of csrc/hipk_sparse_pat.hip and of the windowed tile kernel of csrc/hipk_sparse.hip),
hipk_cheb_update and hipk_csr_gershgorin (csrc/hipk_cheb.hip), each against numpy on inputs chosen so that nothing cancels
or coincides: independent normal panels, four distinct nonzero coefficients that differ from column to column, four leading
dimensions that differ from each other and from m, NaN in every padding row and in the column behind the block.

The fused step is held to a DERIVED bound per element (both kernels accumulate the row sum in double and round once to T):
    |out_i - ref_i| <= B_i = u_T |ref_i| + 2 (len_i + 4) 2^-53 S_i,   S_i = |cy||yk_i| + |cp||yp_i| + |cx||x_i| + |cw| sum_j |a_ij||yk_j|
with ref in np.longdouble from the inputs as rounded to T, u_T = 2^-53 / 2^-24, len_i the length of row i: at most len_i + 4
operations act on partial sums bounded by S_i, the factor 2 covers the summation tree and the gamma_n slack.  The largest
err/B of every case goes to profiles/cheb_step_accuracy.txt.

Which case is there for which branch (chunk = 512 rows of the row-pattern kernel, J = workgroups per XCD, per = chunks per XCD):
  row-pattern form (hipk_set_spmv_format(1), format 2)
    lap1d_8192      width 3; 16 full chunks and no ragged one; the last pair (interior row, last row) is in the buffer-addressed
                    form and its first row references the last column: `near`
    lap2d_33x512    width 5; full chunks only; `near` (row n - 1 - 33 is even, its +33 entry is the last column)
    lap2d_37x41     width 5; two full chunks and a ragged one (the guarded form)
    lap3d_16x17x19  width 7; 5168 rows = 11 chunks on a grid of 8: per = 2 > J = 1, the multi-trip loop (c += J, the prefetch
                    of the next trip's pattern bytes) with a ragged chunk in the second trip
    lattice5        width 5; 40003 rows, 6 patterns with unequal values, second trips in the first workgroup of each XCD
    lattice8        width 8 (PATL(8) / PATC(8)); 6001 rows = 12 chunks, multi-trip; non-symmetric, eight different values in a
                    row, two site types: a transposed read or a permuted table entry changes the result
    (`near` reloads the first row of a pair of two patterns entry by entry, because the pair's 16-byte access may reach one
    element past x.  On gfx950 the descriptor's range check acts per dword and the in-range half of such an access arrives
    intact, so forcing `near` to false changes no bit here; a wrong offset in the reload fails lap1d_8192, lap2d_33x512 and
    lap3d_16x17x19 — the branch runs and is checked, its absence cannot be seen on this part.)
  row-tile form (hipk_set_spmv_format(0), format 0; tests/test_kernels_gpu.py: _csr_cases)
    banded          windowed tiles, 16-bit indices, non-symmetric
    ragged          gather tiles (win == false), a 4000-entry row (nz > TILE_NNZ: the long-row branch), rows without entries
    empty_tiles     tiles without a nonzero: the step still writes cy yk + cp yp + cx x there
    zero_matrix     no nonzero at all: the result is the combination without the product
    lap3d           (37, 41, 29): windows too wide for the LDS buffer, gather tiles with 16-bit indices
    wide32          70 001 rows, two entries per row, a column reach above 65535: 32-bit indices (C16 == false)
  every case runs nx = 1, 2 (NC = 2), 3, 5 (NC = 4 with a partial last group) and 8, in double and float, with Out apart from
  Yprev, Out == Yprev, and Yprev == NULL.
  hipk_cheb_update: grid_cap (m just above num_cu * 8 * per rows, 16-byte and scalar path: blockIdx.x indexing, the cap, the
  grid-stride loop), one misaligned panel (scalar fallback), every subset of {W, Yk, Yprev}, Out on each input, nx = 1 and 8.
  hipk_csr_gershgorin: more than num_cu * 8 * 256 rows (grid-stride loop over the rows, second-stage loop over more than 256
  partial pairs), HIPK_F32 / HIPK_C64 / HIPK_C32, a slab with row0 > 0, rows without a diagonal entry, an empty slab."""
import ctypes as C
import os

import numpy as np
import pytest

import cheb_cases as CC
from kernel_harness import Dev, NPDT
from primme_amd import _ffi as F
from primme_amd import problems
from test_kernels_gpu import _csr_cases, _lattice_csr, _lattice8_csr

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ACCURACY_LOG = os.path.join(ROOT, "profiles", "cheb_step_accuracy.txt")
L = np.longdouble
NXS = (1, 2, 3, 5, 8)
PAT_CASES = ["lap1d_8192", "lap2d_33x512", "lap2d_37x41", "lap3d_16x17x19", "lattice5", "lattice8"]
TILE_CASES = ["banded", "ragged", "empty_tiles", "zero_matrix", "lap3d", "wide32"]
DTYPES = [F.HIPK_F64, F.HIPK_F32]


def _u(npdt):
    return 2.0 ** -53 if np.dtype(npdt) in (np.dtype(np.float64), np.dtype(np.complex128)) else 2.0 ** -24


def _real(npdt):
    return np.dtype(npdt).type(0).real.dtype


@pytest.fixture(scope="module")
def accuracy_log():
    """The step cases add their figures; a run of the whole sweep rewrites profiles/cheb_step_accuracy.txt when the module is done."""
    lines = []
    yield lines
    if len(lines) >= 2 * (len(PAT_CASES) + len(TILE_CASES)):
        with open(ACCURACY_LOG, "w") as f:
            f.write("hipk_csr_cheb_step, one call against the np.longdouble reference: largest |out - ref| / B over nx = 1, 2, 3, 5, 8,\n"
                    "Out apart from Yprev / Out == Yprev / Yprev == NULL;  B_i = u_T |ref_i| + 2 (len_i + 4) 2^-53 S_i\n"
                    "(float: the one rounding of the double result to float is up to half an ulp, which is u_T |ref| for a value just above\n"
                    "a power of two, so among thousands of elements the ratio comes as close to 1 as it can; the double term is what is left\n"
                    "for the arithmetic, and the double rows show how much of it is used)\n")
            f.write("\n".join(sorted(lines)) + "\n")


@pytest.fixture(scope="module")
def num_cu(built):
    import torch
    return int(torch.cuda.get_device_properties(0).multi_processor_count)


@pytest.fixture(scope="module")
def tile_cases():
    cases = {name: (rp, ci, va, n) for name, rp, ci, va, n in _csr_cases()}
    # no 16-bit index stream: the second entry of the first rows lies 66 000 columns to the right of the diagonal
    n = 70001
    rng = np.random.default_rng(5)
    far = (np.arange(n) + 66000) % n
    ci = np.sort(np.stack([np.arange(n), far], axis=1), axis=1).reshape(-1).astype(np.int32)
    cases["wide32"] = (np.arange(0, 2 * n + 1, 2, dtype=np.int32), ci, rng.standard_normal(2 * n), n)
    return cases


def _pat_case(name):
    if name == "lap1d_8192": return problems.laplacian_csr((8192,))
    if name == "lap2d_33x512": return problems.laplacian_csr((33, 512))
    if name == "lap2d_37x41": return problems.laplacian_csr((37, 41))
    if name == "lap3d_16x17x19": return problems.laplacian_csr((16, 17, 19))
    if name == "lattice5": return _lattice_csr(40003, None) + (40003,)
    return _lattice8_csr(6001) + (6001,)


def _pat_trips(n, num_cu):
    """Chunks walked by the busiest workgroup: hipk_pat_grid and pat_kernel's schedule restated (HIPK_PAT_RPL = 1: chunks of 512
    rows; HIPK_PAT_WPS = 6 workgroups per CU; a grid that is a multiple of 8, XCD q owns `per` consecutive chunks and its J
    workgroups walk them with stride J)."""
    nch = (n + 511) // 512
    g = max(8, min(num_cu * 6, nch) // 8 * 8)
    J, per = g // 8, (nch + 7) // 8
    return per, J, -(-min(per, nch) // J)


class _Panel:
    """ncols columns of m rows, ld apart, behind `off` leading REAL elements, and one more column behind the block; everything that
    is not an element of the block holds NaN.  a == None: the block holds NaN too."""

    def __init__(self, side, a, ld, off=0, shape=None):
        m, nc = a.shape if a is not None else shape[:2]
        dtype = a.dtype if a is not None else shape[2]
        self.side, self.m, self.nc, self.ld, self.dtype = side, m, nc, ld, np.dtype(dtype)
        self.f = 2 if self.dtype.kind == "c" else 1          # real elements per element
        rdt = _real(dtype)
        self.off = off
        self.img = np.full(off + (nc + 1) * ld * self.f, np.nan, dtype=rdt)
        if a is not None:
            self._block(self.img)[:nc, :m] = np.ascontiguousarray(a.T)
        self.t = side.arr(self.img)
        self.ptr = side.ptr(self.t, off)

    def _block(self, img):
        v = img[self.off:]
        return (v.view(self.dtype) if self.f == 2 else v).reshape(self.nc + 1, self.ld)

    def read(self):
        """(the block, the whole buffer as it is on the device)"""
        got = self.side.get(self.t)
        return self._block(got)[:self.nc, :self.m].T.copy(), got

    def outside_unchanged(self, got, nx=None):
        a, b = got.copy(), self.img.copy()
        self._block(a)[:self.nc if nx is None else nx, :self.m] = 0
        self._block(b)[:self.nc if nx is None else nx, :self.m] = 0
        return np.array_equal(a.view(np.uint8), b.view(np.uint8))

    def unchanged(self):
        return np.array_equal(self.side.get(self.t).view(np.uint8), self.img.view(np.uint8))


def _coef():
    """cy, cp, cx, cw: distinct, nonzero, another quadruple in every column"""
    cf = F.HipkChebCoef()
    c = np.arange(8)
    cy, cp, cx, cw = 0.7 + 0.1 * c, -0.3 - 0.05 * c, 1.3 + 0.2 * c, -0.45 - 0.03 * c
    for i in range(8):
        cf.cy[i], cf.cp[i], cf.cx[i], cf.cw[i] = cy[i], cp[i], cx[i], cw[i]
    return cf, (cy, cp, cx, cw)


def _create(side, dt, rp, ci, va, n, nloc=None, row0=0):
    A = C.c_void_p()
    rp, ci = np.ascontiguousarray(rp, dtype=np.int32), np.ascontiguousarray(ci, dtype=np.int32)
    vv = np.ascontiguousarray(va, dtype=NPDT[dt])
    assert side.lib.hipk_csr_create(side.ctx, dt, n if nloc is None else nloc, n, row0, rp.ctypes.data_as(C.c_void_p), ci.ctypes.data_as(C.c_void_p),
                                    vv.ctypes.data_as(C.c_void_p), C.byref(A)) == 0
    return A


def _declare(lib):
    lib.hipk_set_spmv_format.argtypes = [C.c_int]
    lib.hipk_csr_format.argtypes = [C.c_void_p]
    lib.hipk_csr_index_bytes.argtypes = [C.c_void_p]


def _step_reference(rp, ci, vat, Yk, Yp, X, coefs):
    """ref and S with and without the Yprev term, in np.longdouble, all 8 columns (column c of a narrower block is the same)."""
    n = len(rp) - 1
    cy, cp, cx, cw = (np.asarray(c).astype(L) for c in coefs)
    yk, yp, x = Yk.astype(L), Yp.astype(L), X.astype(L)
    prod = vat.astype(L)[:, None] * yk[ci]
    Ay, aAy = np.zeros((n, Yk.shape[1]), dtype=L), np.zeros((n, Yk.shape[1]), dtype=L)
    ne = np.diff(rp) > 0
    if prod.shape[0]:
        Ay[ne] = np.add.reduceat(prod, rp[:-1][ne], axis=0)
        aAy[ne] = np.add.reduceat(np.abs(prod), rp[:-1][ne], axis=0)
    ref0 = cy * yk + cx * x + cw * Ay
    S0 = np.abs(cy) * np.abs(yk) + np.abs(cx) * np.abs(x) + np.abs(cw) * aAy
    return {True: (ref0 + cp * yp, S0 + np.abs(cp) * np.abs(yp)), False: (ref0, S0)}


def _run_step_case(lib, side, A, csr, dt, label, accuracy_log, pair=False):
    rp, ci, va, n = csr
    npdt = NPDT[dt]
    rng = np.random.default_rng(n + 7)
    Yk, Yp, X = (rng.standard_normal((n, 8)).astype(npdt) for _ in range(3))
    cf, coefs = _coef()
    refs = _step_reference(rp, ci, np.asarray(va).astype(npdt), Yk, Yp, X, coefs)
    lens = np.diff(rp).astype(L)[:, None]
    ldx, ldk, ldp, ldo = n + 3, n + 5, n + 8, n + 13
    st = lib.hipk_ctx_stream(side.ctx)
    worst = 0.0
    for nx in NXS:
        px, pk = _Panel(side, X[:, :nx], ldx), _Panel(side, Yk[:, :nx], ldk)
        for variant in ("apart", "inplace", "noprev"):
            pp = _Panel(side, Yp[:, :nx], ldp) if variant != "noprev" else None
            po = pp if variant == "inplace" else _Panel(side, None, ldo, shape=(n, nx, npdt))
            lo = ldp if variant == "inplace" else ldo
            assert lib.hipk_csr_cheb_step(A, None, nx, C.byref(cf), px.ptr, ldx, pk.ptr, ldk, pp.ptr if pp else None, ldp, po.ptr, lo) == 0
            out, raw = po.read()
            tag = f"{label} nx={nx} {variant}"
            assert not np.any(np.isnan(out)), tag
            assert po.outside_unchanged(raw), tag             # padding rows m..ld and column nx: bit for bit
            assert px.unchanged() and pk.unchanged() and (variant != "apart" or pp.unchanged()), tag
            ref, S = refs[variant != "noprev"]
            ref, S = ref[:, :nx], S[:, :nx]
            B = _u(npdt) * np.abs(ref) + 2 * (lens + 4) * L(2.0) ** -53 * S
            err = np.abs(out.astype(L) - ref)
            ratio = float(np.max(np.where(B > 0, err / np.where(B > 0, B, 1), np.where(err > 0, np.inf, 0))))
            print(f"{tag}: err/B = {ratio:.3f}")
            worst = max(worst, ratio)
            assert np.all(err <= B), (tag, ratio)
            if pair and variant != "inplace":
                # the pair the fused step replaces: the product a column at a time in the same form, then hipk_cheb_update.  Both run
                # cx x -> fma(cy, yk) -> fma(cp, yp) -> fma(cw, row sum) on the same double row sum: bit for bit in double
                pw, pq = _Panel(side, None, n + 17, shape=(n, nx, npdt)), _Panel(side, None, n + 21, shape=(n, nx, npdt))
                es = np.dtype(npdt).itemsize
                for c in range(nx):
                    assert lib.hipk_csr_matvec(A, None, C.c_void_p(pk.ptr.value + c * ldk * es), ldk, C.c_void_p(pw.ptr.value + c * (n + 17) * es), n + 17, 1) == 0
                assert lib.hipk_cheb_update(st, dt, n, nx, C.byref(cf), px.ptr, ldx, pw.ptr, n + 17, pk.ptr, ldk, pp.ptr if pp else None, ldp,
                                            pq.ptr, n + 21) == 0
                assert np.array_equal(pq.read()[0], out), tag
    accuracy_log.append(f"{label:34s} rows={n:6d} longest row={int(np.max(np.diff(rp))) if n else 0:5d}  max err/B = {worst:.4f}")


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("case", PAT_CASES)
def test_fused_step_row_pattern_form(built, accuracy_log, num_cu, case, dt):
    """One call of hipk_csr_cheb_step in the row-pattern form against the longdouble reference, every element within B_i; in
    double also bit for bit against hipk_csr_matvec (same form, a column at a time) followed by hipk_cheb_update."""
    rp, ci, va, n = _pat_case(case)
    if case in ("lap3d_16x17x19", "lattice8", "lattice5"):
        per, J, trips = _pat_trips(n, num_cu)
        assert per > J and trips >= 2, (per, J, trips)       # the multi-trip loop runs
    side = Dev()
    lib = side.lib
    _declare(lib)
    old = lib.hipk_set_spmv_format(1)
    try:
        A = _create(side, dt, rp, ci, va, n)
        assert lib.hipk_csr_format(A) == 2
        _run_step_case(lib, side, A, (rp, ci, va, n), dt, f"pattern {case} {np.dtype(NPDT[dt]).name}", accuracy_log, pair=dt == F.HIPK_F64)
        lib.hipk_csr_destroy(A)
    finally:
        lib.hipk_set_spmv_format(old)
        side.close()


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("case", TILE_CASES)
def test_fused_step_row_tile_form(built, accuracy_log, tile_cases, case, dt):
    """The same in the row-tile form: the windowed block kernel with its gather, long-row and empty-row branches."""
    rp, ci, va, n = tile_cases[case]
    side = Dev()
    lib = side.lib
    _declare(lib)
    old = lib.hipk_set_spmv_format(0)
    try:
        A = _create(side, dt, rp, ci, va, n)
        assert lib.hipk_csr_format(A) == 0
        assert lib.hipk_csr_index_bytes(A) == (4 if case == "wide32" else 2)
        _run_step_case(lib, side, A, (rp, ci, va, n), dt, f"tile    {case} {np.dtype(NPDT[dt]).name}", accuracy_log)
        lib.hipk_csr_destroy(A)
    finally:
        lib.hipk_set_spmv_format(old)
        side.close()


def test_fused_step_return_codes(built):
    """1 = no fused form (a complex matrix, a stencil handle, a row slab with halo, a rectangular operator); -1 = nx = 9, Out == Yk,
    NULL X; 0 with nothing written for nx = 0."""
    side = Dev()
    lib = side.lib
    _declare(lib)
    cf, _ = _coef()
    n, ld = 600, 700
    rng = np.random.default_rng(1)
    px, pk, pp = (_Panel(side, rng.standard_normal((n, 9)), ld) for _ in range(3))
    po = _Panel(side, None, ld, shape=(n, 9, np.float64))
    pz = [_Panel(side, (rng.standard_normal((n, 2)) + 1j * rng.standard_normal((n, 2))), ld) for _ in range(4)]

    def step(A, nx, x, yk, yp, out):
        return lib.hipk_csr_cheb_step(A, None, nx, C.byref(cf), x.ptr if x else None, ld, yk.ptr, ld, yp.ptr, ld, out.ptr, ld)
    try:
        made = []
        rp, ci, va = problems.hermitian_banded_csr(n)[:3]
        made.append(_create(side, F.HIPK_C64, rp, ci, va, n))
        assert step(made[-1], 2, pz[0], pz[1], pz[2], pz[3]) == 1
        A = C.c_void_p()
        assert lib.hipk_stencil_create(side.ctx, F.HIPK_F64, 20, 30, 1, 0, n, C.byref(A)) == 0
        made.append(A)
        assert step(A, 2, px, pk, pp, po) == 1
        rp, ci, va, ng = problems.laplacian_csr((20, 60), row0=300, nrows=n)
        made.append(_create(side, F.HIPK_F64, rp, ci, va, ng, nloc=n, row0=300))
        assert lib.hipk_csr_halo_lo(made[-1]) > 0
        assert step(made[-1], 2, px, pk, pp, po) == 1
        rp, ci, va, _ = problems.laplacian_csr((n,))
        A = C.c_void_p()
        rpr = np.ascontiguousarray(rp[:n - 99])
        assert lib.hipk_csr_create_rect(side.ctx, F.HIPK_F64, n - 100, n, rpr.ctypes.data_as(C.c_void_p), ci.ctypes.data_as(C.c_void_p),
                                        va.ctypes.data_as(C.c_void_p), C.byref(A)) == 0
        made.append(A)
        assert step(A, 2, px, pk, pp, po) == 1
        made.append(_create(side, F.HIPK_F64, rp, ci, va, n))
        A = made[-1]
        assert step(A, 9, px, pk, pp, po) == -1
        assert step(A, 2, px, pk, pp, pk) == -1
        assert step(A, 2, None, pk, pp, po) == -1
        assert step(A, 0, px, pk, pp, po) == 0
        assert po.unchanged() and pp.unchanged() and pk.unchanged()     # nothing written by any of the calls above
        assert step(A, 2, px, pk, pp, po) == 0                # and the same arguments with nx = 2 do run
        assert not np.any(np.isnan(po.read()[0][:, :2]))
        for A in made:
            lib.hipk_csr_destroy(A)
    finally:
        side.close()


# ---- hipk_cheb_update ---------------------------------------------------------------------------------------------------
ALL_DT = [F.HIPK_F64, F.HIPK_F32, F.HIPK_C64, F.HIPK_C32]
_NAMES = ("X", "W", "Yk", "Yp")


def _normal(rng, m, nx, npdt):
    a = rng.standard_normal((m, nx))
    if np.dtype(npdt).kind == "c":
        a = a + 1j * rng.standard_normal((m, nx))
    return a.astype(npdt)


def _update_check(side, dt, m, nx, lds, present=("W", "Yk", "Yp"), out_on=None, offs=None, seed=0):
    """One call of hipk_cheb_update against numpy in float64 / complex128 with the bound u_T |ref| + 2 * 5 * 2^-53 * S per real
    component (4 products and 3 additions in double, one rounding to T).  lds: leading dimensions of X, W, Yk, Yp, Out in
    elements; present: which of W, Yk, Yp are passed (the others are NULL, their coefficients stay nonzero); out_on: the input Out
    aliases; offs: leading real elements of a panel (alignment)."""
    lib = side.lib
    npdt = NPDT[dt]
    rng = np.random.default_rng(100 + seed)
    offs = offs or {}
    cf, (cy, cp, cx, cw) = _coef()
    data = {k: _normal(rng, m, nx, npdt) for k in _NAMES}
    pan = {k: _Panel(side, data[k], lds[i], off=offs.get(k, 0)) for i, k in enumerate(_NAMES) if k == "X" or k in present}
    if out_on:
        po, ldo = pan[out_on], lds[_NAMES.index(out_on)]
    else:
        po, ldo = _Panel(side, None, lds[4], off=offs.get("Out", 0), shape=(m, nx, npdt)), lds[4]
    wide = np.complex128 if np.dtype(npdt).kind == "c" else np.float64
    f = 2 if np.dtype(npdt).kind == "c" else 1
    ref, S = 0, 0                                             # S per real component: (re, im) side by side
    for k, c in (("X", cx), ("Yk", cy), ("Yp", cp), ("W", cw)):
        if k in pan:
            ref = ref + c[:nx] * data[k].astype(wide)
            S = S + np.repeat(np.abs(c[:nx]), f) * np.abs(data[k].astype(wide).view(np.float64))

    def p(k):
        return (pan[k].ptr if k in pan else None), lds[_NAMES.index(k)]
    st = lib.hipk_ctx_stream(side.ctx)
    assert lib.hipk_cheb_update(st, dt, m, nx, C.byref(cf), *p("X"), *p("W"), *p("Yk"), *p("Yp"), po.ptr, ldo) == 0
    out, raw = po.read()
    assert not np.any(np.isnan(out.view(_real(npdt))))
    assert po.outside_unchanged(raw)                          # padding rows and the column behind the block: bit for bit
    for k in pan:
        assert k == out_on or pan[k].unchanged(), k
    refr = ref.view(np.float64)                               # complex: (re, im) side by side, as S
    err = np.abs(out.astype(wide).view(np.float64) - refr)
    B = _u(npdt) * np.abs(refr) + 2 * 5 * 2.0 ** -53 * S
    assert np.all(err <= B), float(np.max(err / B))


@pytest.mark.parametrize("path", ["wide", "scalar"])
@pytest.mark.parametrize("dt", ALL_DT)
def test_update_grid_cap_and_stride(built, num_cu, dt, path):
    """More rows than num_cu * 8 workgroups cover in their two trips per lane: the grid is capped, blockIdx.x indexes the rows and
    the grid-stride loop runs a third, partial trip that ends in a workgroup in the middle of the grid.  m odd: on the 16-byte
    path the rows past the last full access run as well (they belong to the first lanes of the first workgroup)."""
    npdt = NPDT[dt]
    f = 2 if np.dtype(npdt).kind == "c" else 1
    vw = 16 // np.dtype(_real(npdt)).itemsize
    per = 256 * (vw if path == "wide" else 1) * 2             # real elements per workgroup: cheb_update_t
    m = (num_cu * 8 * per + per * 40 + per // 2) // f + 1
    assert m % 2 == 1 and m * f > num_cu * 8 * per
    ld0 = (m + 8) // 4 * 4                                    # every column starts on a 16-byte boundary ...
    lds = [ld0 + 4 * i for i in range(5)]
    side = Dev()
    try:
        # ... and on the scalar path Yk one real element behind one
        _update_check(side, dt, m, 2, lds, out_on="Yp", offs={"Yk": 1} if path == "scalar" else None, seed=dt)
    finally:
        side.close()


@pytest.mark.parametrize("dt", ALL_DT)
def test_update_one_misaligned_panel(built, dt):
    """One panel starts one real element off a 16-byte boundary, the other four on one: the scalar path serves the call."""
    side = Dev()
    try:
        m, nx = 1537, 3
        lds = [1540, 1544, 1548, 1552, 1556]
        for i, k in enumerate(_NAMES + ("Out",)):
            _update_check(side, dt, m, nx, lds, offs={k: 1}, seed=i)
        _update_check(side, dt, m, nx, lds, seed=9)           # all aligned, m odd: 16-byte path with its tail
    finally:
        side.close()


@pytest.mark.parametrize("dt", ALL_DT)
def test_update_panel_subsets_and_aliasing(built, dt):
    """Every subset of {W, Yk, Yprev} present or NULL (the coefficients of the missing ones are nonzero and must be ignored), Out on
    each present input in turn, nx = 1 and 8, on the 16-byte path (lds multiples of 4) and the scalar one (odd lds)."""
    side = Dev()
    try:
        m = 1001
        for lds in ([1004, 1008, 1012, 1016, 1020], [1003, 1006, 1009, 1014, 1019]):
            for mask in range(8):
                present = tuple(k for b, k in enumerate(("W", "Yk", "Yp")) if mask >> b & 1)
                _update_check(side, dt, m, 3, lds, present=present, seed=mask)
            for nx in (1, 8):
                for k in _NAMES:
                    _update_check(side, dt, m, nx, lds, out_on=k, seed=nx)
                _update_check(side, dt, m, nx, lds, seed=nx + 1)
    finally:
        side.close()


# ---- hipk_csr_gershgorin ------------------------------------------------------------------------------------------------
def _gersh_lattice(n, dtype, lo_row, hi_row):
    """3 entries per row, values multiples of 1/8 (complex: multiples of (3 + 4i)/8, moduli exact; the diagonal carries an imaginary
    part that must be ignored): every row sum is exact in float and double.  Rows lo_row / hi_row hold the global minimum /
    maximum."""
    i = np.arange(n)
    cols = np.stack([i - 1, i, i + 1], axis=1)
    left, right = -(1 + i % 3) / 8.0, (2 + i % 4) / 8.0
    diag = 2.0 + (i % 5) / 8.0
    diag[lo_row], diag[hi_row] = -50.0, 50.0
    vals = np.stack([left, diag, right], axis=1)
    if np.dtype(dtype).kind == "c":
        vals = vals * np.array([3 + 4j, 1, 3 - 4j]) + np.array([0, 0.625j, 0])
    keep = (cols >= 0) & (cols < n)
    rp = np.zeros(n + 1, dtype=np.int32); np.cumsum(keep.sum(axis=1), out=rp[1:])
    return rp, cols[keep].astype(np.int32), vals[keep].astype(dtype)


def _gershgorin(side, A):
    out = (C.c_double * 2)()
    assert side.lib.hipk_csr_gershgorin(A, None, out) == 0
    return out[0], out[1]


@pytest.mark.parametrize("swap", [False, True])
def test_gershgorin_grid_stride_and_second_stage(built, num_cu, swap):
    """More rows than the capped grid has lanes (the grid-stride loop over the rows) and more than 256 partial pairs (the second
    stage's loop); the minimum in the last row, which a second trip serves, the maximum in the middle of the 300th workgroup,
    and the two swapped.  Exact equality: every sum is exact."""
    n = num_cu * 8 * 256 + 1000 * 256 + 77
    rows = (n - 1, 299 * 256 + 128)
    rp, ci, va = _gersh_lattice(n, np.float64, *(rows[::-1] if swap else rows))
    side = Dev()
    try:
        A = _create(side, F.HIPK_F64, rp, ci, va, n)
        assert _gershgorin(side, A) == CC.gershgorin_numpy(rp, ci, va, n)
        side.lib.hipk_csr_destroy(A)
    finally:
        side.close()


@pytest.mark.parametrize("dt", [F.HIPK_F32, F.HIPK_C64, F.HIPK_C32])
def test_gershgorin_dtypes(built, dt):
    n = 70001                                                 # 274 workgroups: the second stage's loop runs here too
    side = Dev()
    try:
        for rows in ((n - 1, 199 * 256 + 128), (271 * 256 + 3, 0)):
            rp, ci, va = _gersh_lattice(n, NPDT[dt], *rows)
            A = _create(side, dt, rp, ci, va, n)
            want = CC.gershgorin_numpy(rp, ci, va, n)
            assert want[0] < -50 and want[1] > 50
            assert _gershgorin(side, A) == want
            side.lib.hipk_csr_destroy(A)
    finally:
        side.close()


def test_gershgorin_row_slab_offdiagonal_and_empty(built):
    side = Dev()
    try:
        # rows [2000, 5003) of an 8000-column matrix: the diagonal of local row i is column 2000 + i; column i — the local
        # row number — holds an off-diagonal entry, which a test against i would take for the diagonal
        row0, nloc, n = 2000, 3003, 8000
        i = np.arange(nloc)
        ci = np.stack([i, row0 + i, row0 + i + 1], axis=1).reshape(-1).astype(np.int32)
        va = np.stack([(1 + i % 7) / 8.0, 3.0 - (i % 11) / 8.0, -(2 + i % 5) / 8.0], axis=1).reshape(-1)
        rp = np.arange(0, 3 * nloc + 1, 3, dtype=np.int32)
        want = CC.gershgorin_numpy(rp, ci - row0, va, nloc)
        assert want != CC.gershgorin_numpy(rp, ci, va, nloc)
        for dt in (F.HIPK_F64, F.HIPK_F32):
            A = _create(side, dt, rp, ci, va, n, nloc=nloc, row0=row0)
            assert _gershgorin(side, A) == want
            side.lib.hipk_csr_destroy(A)
        # no diagonal entry: d = 0, the bounds are -+ the largest absolute row sum
        ci2 = np.stack([(i + 1) % nloc, (i + 5) % nloc], axis=1).reshape(-1).astype(np.int32)
        va2 = np.stack([(1 + i % 9) / 8.0, -(3 + i % 13) / 8.0], axis=1).reshape(-1)
        rp2 = np.arange(0, 2 * nloc + 1, 2, dtype=np.int32)
        A = _create(side, F.HIPK_F64, rp2, ci2, va2, nloc)
        s = float(np.max(np.abs(va2).reshape(-1, 2).sum(axis=1)))
        assert _gershgorin(side, A) == (-s, s) == CC.gershgorin_numpy(rp2, ci2, va2, nloc)
        side.lib.hipk_csr_destroy(A)
        # a slab of zero rows: the neutral element of the reduction across ranks
        A = _create(side, F.HIPK_F64, np.zeros(1, dtype=np.int32), np.zeros(1, dtype=np.int32), np.zeros(1), n, nloc=0, row0=row0)
        assert _gershgorin(side, A) == (np.inf, -np.inf)
        side.lib.hipk_csr_destroy(A)
    finally:
        side.close()
