"""Matrices and helpers shared by tests/test_kernels_gpu.py (the device CSR products) and tests/test_csr_plan_host.py (the host
analysis of the row tiles, csrc/csr_tools.c: primme_amd_csr_tile_plan).  Not a test module."""
import ctypes as C

import numpy as np

from primme_amd import _ffi as F
from primme_amd import problems

TILE_NNZ, TILE_ROWS, TILE_WINDOW = 2048, 256, 3072          # include/primme_amd_io.h


def csr_cases():
    """name, rp, ci, va, n of the six matrices the CSR product tests run"""
    rp, ci, va, n = problems.laplacian_csr((37, 41, 29))
    yield "lap3d", rp, ci, va, n
    rp, ci, va, n = problems.laplacian_csr((300, 211))
    yield "lap2d", rp, ci, va, n
    # banded, ~17 nonzeros per row inside a +-40 band: every tile's column window is narrow, which is the
    # case the LDS-windowed block kernel takes (block-diagonal / banded matrices, BASELINE configs[2])
    rng = np.random.default_rng(8)
    n = 30011
    rows = np.repeat(np.arange(n), 17)
    cols = np.clip(rows + rng.integers(-40, 41, size=rows.size), 0, n - 1)
    key = np.unique(rows.astype(np.int64) * n + cols)
    rows, cols = (key // n).astype(np.int64), (key % n).astype(np.int32)
    rp = np.zeros(n + 1, dtype=np.int64); np.add.at(rp, rows + 1, 1); rp = np.cumsum(rp)
    yield "banded", rp.astype(np.int32), cols, rng.standard_normal(cols.size), n
    # ragged: empty rows, one very long row (> LDS tile), random short rows
    rng = np.random.default_rng(2)
    n = 5000
    counts = rng.integers(0, 9, size=n)
    counts[17] = 0; counts[18] = 0; counts[100] = 4000; counts[n - 1] = 0
    rp = np.zeros(n + 1, dtype=np.int64); np.cumsum(counts, out=rp[1:])
    ci = np.concatenate([np.sort(rng.choice(n, size=c, replace=False)) for c in counts]).astype(np.int32)
    va = rng.standard_normal(len(ci))
    yield "ragged", rp.astype(np.int32), ci, va, n
    # all-empty tiles: 300 empty rows first (the first tile has no nonzero), 600 in the middle, 700 at the end (those
    # tiles' clamped loads land on the padded element behind the last nonzero); and a matrix without any nonzero
    rng = np.random.default_rng(3)
    n = 3000
    counts = rng.integers(1, 7, size=n)
    counts[:300] = 0; counts[1200:1800] = 0; counts[n - 700:] = 0
    rp = np.zeros(n + 1, dtype=np.int64); np.cumsum(counts, out=rp[1:])
    ci = np.concatenate([np.sort(rng.choice(n, size=c, replace=False)) for c in counts if c]).astype(np.int32)
    yield "empty_tiles", rp.astype(np.int32), ci, rng.standard_normal(len(ci)), n
    yield "zero_matrix", np.zeros(601, dtype=np.int32), np.zeros(0, dtype=np.int32), np.zeros(0), 600


class Plan:
    """numpy copies of a primme_amd_tile_plan"""

    def __init__(self, P, nrows, nnz, dtype):
        nt = P.ntiles
        take = lambda ptr, ct, cnt: np.ctypeslib.as_array(C.cast(ptr, C.POINTER(ct)), shape=(max(cnt, 1),))[:cnt].copy()
        self.ntiles, self.cw_max, self.windowed = nt, P.cw_max, P.windowed
        self.halo_lo, self.halo_hi, self.c16back = P.halo_lo, P.halo_hi, P.c16back
        self.tiles = take(P.tiles, C.c_int32, nt + 1)
        self.info = take(P.info, C.c_int32, 4 * (nt + 1)).reshape(nt + 1, 4)
        self.win = take(P.win, C.c_int32, 2 * (nt + 1)).reshape(nt + 1, 2)
        self.diag = take(P.diag, C.c_uint8, nrows * np.dtype(dtype).itemsize).view(dtype)
        self.col16 = take(P.col16, C.c_uint16, nnz + 1) if P.col16 else None


def tile_plan(lib, rp, ci, va, row0=0, x0=None, xlen=None, ncols_global=None, real=True):
    """-> Plan through primme_amd_csr_tile_plan of `lib`; x0 / xlen default to the row slab, ncols_global to its end"""
    rp = np.ascontiguousarray(rp, dtype=np.int32); ci = np.ascontiguousarray(ci, dtype=np.int32); va = np.ascontiguousarray(va)
    nrows = len(rp) - 1
    x0 = row0 if x0 is None else x0
    xlen = nrows if xlen is None else xlen
    ncols_global = max(row0 + nrows, x0 + xlen) if ncols_global is None else ncols_global
    lib.primme_amd_csr_tile_plan.argtypes = [C.c_int64] * 5 + [C.c_void_p] * 3 + [C.c_size_t, C.c_int, C.POINTER(C.POINTER(F.PrimmeAmdTilePlan))]
    lib.primme_amd_csr_tile_plan.restype = C.c_int
    lib.primme_amd_tile_plan_free.argtypes = [C.POINTER(F.PrimmeAmdTilePlan)]
    lib.primme_amd_tile_plan_free.restype = None
    h = C.POINTER(F.PrimmeAmdTilePlan)()
    rc = lib.primme_amd_csr_tile_plan(nrows, row0, x0, xlen, ncols_global, rp.ctypes.data, ci.ctypes.data, va.ctypes.data, va.dtype.itemsize,
                                      int(real), C.byref(h))
    assert rc == 0 and h
    out = Plan(h.contents, nrows, len(ci), va.dtype)
    lib.primme_amd_tile_plan_free(h)
    return out
