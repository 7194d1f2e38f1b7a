"""Matrices and helpers shared by tests/test_sliced_host.py and tests/test_sliced_gpu.py (the sliced-ELL form, SELL-64-256, of
include/primme_amd_io.h and csrc/hipk_sparse_sell.hip).  Not a test module."""
import ctypes as C
import functools

import numpy as np

from primme_amd import _ffi as F
from primme_amd import problems
import reference_driver_cases as RD

MAX_PADDING = 1.25          # the device operator's limit (csrc/hipk_sparse_sell.hip)


def _csr(n, rows):
    """rows: list of (columns, values) per row -> rp, ci, va"""
    rp = np.zeros(n + 1, dtype=np.int64)
    rp[1:] = np.cumsum([len(c) for c, _ in rows])
    ci = np.concatenate([np.asarray(c, dtype=np.int64) for c, _ in rows] + [np.zeros(0, dtype=np.int64)])
    va = np.concatenate([np.asarray(v, dtype=np.float64) for _, v in rows] + [np.zeros(0)])
    return rp.astype(np.int32), ci.astype(np.int32), va


def band(n, seed=3, drop=0.04, banned=()):
    """random band matrix of half-width 5 with a few entries dropped (interior rows of 7..11 entries: more than the 8 of a row
    pattern, so the device operator does not take the row-pattern form; the diagonal always kept), no entry in the `banned`
    columns (those rows lose their diagonal too).  n = 1: one row that stores its only column nine times (duplicates are
    legal CSR and add up) — with a single entry the device would keep it as a row pattern"""
    rng = np.random.default_rng(seed + n)
    if n == 1: return _csr(1, [([0] * 9, rng.standard_normal(9))])
    rows = []
    for i in range(n):
        cols = [j for j in range(max(0, i - 5), min(n, i + 6)) if (j == i or rng.random() >= drop) and j not in banned]
        rows.append((cols, rng.standard_normal(len(cols)) + (0.5 if len(cols) else 0.0)))
    return _csr(n, rows)


def lunda_tiled(T):
    rp, ci, va, _ = RD.lunda()
    return problems.tile_block_diagonal(rp, ci, va, T, lambda t: 1.0 + t / 1000.0)


def with_empty_rows(n=600):
    """rows 100..179 store nothing: window 0 sorts 80 empty rows to its end, slots 192..255 are an all-empty slice"""
    rp, ci, va = band(n, seed=5, drop=0.0)
    keep = np.ones(len(ci), dtype=bool)
    keep[rp[100]:rp[180]] = False
    lens = np.diff(rp); lens[100:180] = 0
    rp2 = np.zeros(n + 1, dtype=np.int32); rp2[1:] = np.cumsum(lens)
    return rp2, ci[keep], va[keep]


def random_band(n=1000, seed=9):
    """row lengths 0..21 (every length occurs; four rows in five have 18..21 entries, which keeps the padding of the 256-row
    sort under the limit), columns within 40 of the row, in increasing order"""
    rng = np.random.default_rng(seed)
    lens = np.where(rng.random(n) < 0.8, rng.integers(18, 22, size=n), rng.integers(0, 22, size=n))
    lens[:22] = np.arange(22)[::-1]
    rows = []
    for i in range(n):
        lo, hi = max(0, i - 40), min(n, i + 41)
        cols = np.sort(rng.choice(np.arange(lo, hi), size=int(lens[i]), replace=False))
        rows.append((cols, rng.standard_normal(len(cols))))
    return _csr(n, rows)


def wide_tridiagonal(n=70000):
    """tridiagonal + the entry (0, n - 1): slice 0 spans n columns, more than 16 bits hold"""
    rng = np.random.default_rng(12)
    rows = []
    for i in range(n):
        cols = [j for j in (i - 1, i, i + 1) if 0 <= j < n]
        if i == 0: cols.append(n - 1)
        rows.append((cols, None))
    rp = np.zeros(n + 1, dtype=np.int64); rp[1:] = np.cumsum([len(c) for c, _ in rows])
    ci = np.concatenate([np.asarray(c) for c, _ in rows])
    return rp.astype(np.int32), ci.astype(np.int32), rng.standard_normal(len(ci))


def fallback_300():
    """300 rows of 3 entries, row 17 has 250: its slice is 250 wide, the padding far above the limit"""
    rng = np.random.default_rng(14)
    n = 300
    rows = []
    for i in range(n):
        cols = np.arange(250) + 20 if i == 17 else np.array(sorted({max(i - 1, 0), i, min(i + 1, n - 1), (i + 2) % n}))[:3]
        rows.append((cols, rng.standard_normal(len(cols))))
    return _csr(n, rows)


@functools.lru_cache(maxsize=None)
def matrix(name):
    """-> rp, ci, va (double); read-only, shared"""
    if name.startswith("band"): out = band(int(name[4:]))
    elif name == "lunda3": out = lunda_tiled(3)
    elif name == "lunda4": out = lunda_tiled(4)
    elif name == "empty_rows": out = with_empty_rows()
    elif name == "random_band": out = random_band()
    elif name == "wide": out = wide_tridiagonal()
    elif name == "fallback300": out = fallback_300()
    elif name == "holes257": out = band(257, seed=21, banned=(0, 64, 128, 256))
    else: raise ValueError(name)
    for a in out: a.setflags(write=False)
    return out


SHAPES = ["band1", "band64", "band65", "band256", "band257", "lunda3", "empty_rows"]


def padding_numpy(rp):
    """padded entries of SELL-64-256 (stable descending sort inside 256-row windows, slices of 64 slots, a slice as wide as
    its longest row, only the slots that exist counted) -> padded, sorted lengths, perm"""
    lens = np.diff(rp).astype(np.int64)
    m = len(lens)
    padded, slen, perm = 0, np.zeros(m, dtype=np.int64), np.zeros(m, dtype=np.int64)
    for w0 in range(0, m, 256):
        l = lens[w0:w0 + 256]
        order = np.argsort(-l, kind="stable")
        perm[w0:w0 + len(l)] = order; slen[w0:w0 + len(l)] = l[order]
    for s0 in range(0, m, 64):
        padded += int(slen[s0:s0 + 64].max()) * len(slen[s0:s0 + 64])
    return padded, slen, perm


class Sliced:
    """numpy copies of a primme_amd_sliced; None arrays never: to_sliced returns the return code alone when nothing was built"""

    def __init__(self, S, dtype):
        ns, tot = S.nslices, None
        self.m, self.nnz, self.nslices, self.padded, self.idx16 = S.m, S.nnz, ns, S.padded, S.idx16
        take = lambda ptr, ct, cnt: np.ctypeslib.as_array(C.cast(ptr, C.POINTER(ct)), shape=(max(cnt, 1),))[:cnt].copy()
        self.base = take(S.base, C.c_int64, ns + 1)
        tot = int(self.base[ns])
        self.cmin = take(S.cmin, C.c_int32, ns); self.perm = take(S.perm, C.c_uint8, 64 * ns); self.len = take(S.len, C.c_uint16, 64 * ns)
        self.val = take(S.val, C.c_uint8, tot * np.dtype(dtype).itemsize).view(dtype)
        self.idx = take(S.idx, C.c_uint16 if S.idx16 else C.c_int32, tot)


def to_sliced(lib, rp, ci, va, max_padding=MAX_PADDING):
    """-> (rc, Sliced or None) through primme_amd_csr_to_sliced of `lib`"""
    rp = np.ascontiguousarray(rp, dtype=np.int32); ci = np.ascontiguousarray(ci, dtype=np.int32); va = np.ascontiguousarray(va)
    lib.primme_amd_csr_to_sliced.argtypes = [C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_double,
                                             C.POINTER(C.POINTER(F.PrimmeAmdSliced))]
    lib.primme_amd_csr_to_sliced.restype = C.c_int
    lib.primme_amd_sliced_free.argtypes = [C.POINTER(F.PrimmeAmdSliced)]
    lib.primme_amd_sliced_free.restype = None
    h = C.POINTER(F.PrimmeAmdSliced)()
    rc = lib.primme_amd_csr_to_sliced(len(rp) - 1, rp.ctypes.data, ci.ctypes.data, va.ctypes.data, va.dtype.itemsize, max_padding, C.byref(h))
    if rc:
        assert not h
        return rc, None
    out = Sliced(h.contents, va.dtype)
    lib.primme_amd_sliced_free(h)
    return 0, out


L = np.longdouble


def product_reference(rp, ci, va_t, X_t):
    """longdouble A X and S = |A| |X| of the values and vectors as the device holds them -> ref, S (m x k)"""
    m = len(rp) - 1
    rows = np.repeat(np.arange(m), np.diff(rp))
    a = va_t.astype(L)[:, None]
    xg = X_t.astype(L)[ci]
    ref, S = np.zeros((m, X_t.shape[1]), dtype=L), np.zeros((m, X_t.shape[1]), dtype=L)
    np.add.at(ref, rows, a * xg)
    np.add.at(S, rows, np.abs(a) * np.abs(xg))
    return ref, S


def product_bound(rp, ref, S, dtype, extra=None):
    """(len_i + 2) 2^-53 S_i: one fma chain of len_i terms in double, + one rounding of the output in float"""
    lens = np.diff(rp).astype(L)[:, None]
    B = (lens + 2) * L(2.0) ** -53 * (S if extra is None else S + extra)
    if np.dtype(dtype) == np.float32: B = B + L(2.0) ** -24 * np.abs(ref)
    return B
