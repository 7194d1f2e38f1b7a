"""The host analysis of the device CSR operator's row tiles (csrc/csr_tools.c: primme_amd_csr_tile_plan, fields in
include/primme_amd_io.h), through the CPU checker library as tests/test_sliced_host.py calls the sliced converter, against a numpy
restatement: the tiles partition the rows, respect both limits unless they are a single row, and are maximal under the greedy
rule; the records are rowptr at the tile bounds; every window is the exact min / max of the tile's columns or {0, 0}; cw_max,
windowed and the halo extent follow their rules; the 16-bit stream gives every column back and exists exactly when the reach
fits; the diagonal is bit-identical."""
import numpy as np
import pytest

import checkers
import csr_cases as CC

NNZ, ROWS, WINDOW = CC.TILE_NNZ, CC.TILE_ROWS, CC.TILE_WINDOW


def check(P, rp, ci, va, row0=0, x0=None, xlen=None, ncols_global=None, real=True):
    rp = np.asarray(rp, dtype=np.int64); ci = np.asarray(ci, dtype=np.int64)
    nrows = len(rp) - 1
    x0 = row0 if x0 is None else x0
    xlen = nrows if xlen is None else xlen
    ncols_global = max(row0 + nrows, x0 + xlen) if ncols_global is None else ncols_global
    nt, t = P.ntiles, P.tiles.astype(np.int64)
    lens = np.diff(rp)
    # the tiles partition the rows
    assert len(t) == nt + 1 and t[0] == 0 and t[-1] == nrows and np.all(np.diff(t) > 0)
    nz, nr = rp[t[1:]] - rp[t[:-1]], np.diff(t)
    # both limits unless a single row; maximal under the greedy rule: the next row did not fit
    assert np.all(((nz <= NNZ) & (nr <= ROWS)) | (nr == 1))
    nxt = lens[t[1:-1]] if nt > 1 else np.zeros(0, dtype=np.int64)
    assert np.all((nr[:-1] == ROWS) | (nz[:-1] + nxt > NNZ))
    # the records: rowptr at the tile bounds, and one zero record behind the last tile
    assert np.array_equal(P.info[:nt], np.stack([t[:-1], t[1:], rp[t[:-1]], rp[t[1:]]], axis=1))
    assert not P.info[nt].any() and not P.win[nt].any()
    # halo extent
    lo = int(max(0, (x0 - ci).max())) if len(ci) else 0
    hi = int(max(0, (ci - (x0 + xlen) + 1).max())) if len(ci) else 0
    assert (P.halo_lo, P.halo_hi) == (lo, hi)
    # windows: the exact min / max of the tile's columns when they lie inside the owned entries and span <= WINDOW
    cw_max, narrow, back, spans = 0, 0, 0, []
    for k in range(nt):
        c = ci[rp[t[k]]:rp[t[k + 1]]]
        want = (0, 0)
        if len(c):
            cmin, cmax = int(c.min()), int(c.max())
            spans.append((k, cmax))
            back = max(back, row0 + int(t[k]) - cmin)
            if cmin >= x0 and cmax < x0 + xlen and cmax - cmin + 1 <= WINDOW:
                want = (cmin, cmax - cmin + 1)
                cw_max = max(cw_max, want[1])
                narrow += want[1] * 8 <= WINDOW
        assert tuple(P.win[k]) == want, k
    assert P.cw_max == cw_max
    assert P.windowed == int(lo == 0 and hi == 0 and nt > 0 and narrow * 10 >= nt * 9)
    # the diagonal: the entry at column row0 + i of row i (0 without one), bit for bit
    va = np.ascontiguousarray(va)
    diag = np.zeros(nrows, dtype=va.dtype)
    rows = np.repeat(np.arange(nrows), lens)
    on = ci == row0 + rows
    diag[rows[on]] = va[on]                                 # (a row's last such entry, as the assignment order gives it)
    assert P.diag.tobytes() == diag.tobytes()
    # the 16-bit stream: exists exactly when every entry fits and the guards hold; gives every column back
    reach = max([cmax - (row0 + int(t[k]) - back) for k, cmax in spans] + [0])
    present = real and nt > 0 and reach <= 65535 and row0 - back > -2 ** 30 and ncols_global < 2 ** 31 - 1
    assert (P.col16 is not None) == present
    if present:
        assert P.c16back == back
        tile_of = np.repeat(np.arange(nt), nz)
        assert np.array_equal(ci, row0 + t[tile_of] - P.c16back + P.col16[:len(ci)].astype(np.int64))
        assert P.col16[len(ci)] == 0
    return P


def _from_lens(lens, ncols, seed=0, cols=None):
    """rows of the given lengths, columns increasing from a random start (or `cols(i, len)`), random values"""
    rng = np.random.default_rng(seed)
    rp = np.zeros(len(lens) + 1, dtype=np.int64); rp[1:] = np.cumsum(lens)
    ci = np.concatenate([np.zeros(0, dtype=np.int64)] + [
        (cols(i, l) if cols else rng.integers(0, ncols - l + 1) + np.arange(l)) for i, l in enumerate(lens)])
    return rp.astype(np.int32), ci.astype(np.int32), rng.standard_normal(len(ci))


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_product_test_matrices(built, dtype):
    """the six matrices of the device product tests: narrow windows and a 16-bit stream (lap2d, banded), a 4 000-entry row
    that is a tile of its own (ragged), all-empty tiles, nnz = 0"""
    lib = checkers.load_hostcheck()
    seen = {}
    for name, rp, ci, va, n in CC.csr_cases():
        va = va.astype(dtype)
        seen[name] = P = check(CC.tile_plan(lib, rp, ci, va), rp, ci, va)
        print(f"{name}: {P.ntiles} tiles, cw_max {P.cw_max}, windowed {P.windowed}, col16 {P.col16 is not None}, c16back {P.c16back}")
    assert seen["banded"].windowed == 1 and seen["banded"].col16 is not None and seen["lap2d"].col16 is not None
    R = seen["ragged"]
    k = int(np.searchsorted(R.tiles, 100, side="right")) - 1
    assert (R.tiles[k], R.tiles[k + 1]) == (100, 101) and R.info[k, 3] - R.info[k, 2] == 4000
    E = seen["empty_tiles"]
    assert (E.tiles[0], E.tiles[1]) == (0, 256) and E.info[0, 2] == E.info[0, 3] and tuple(E.win[0]) == (0, 0)
    Z = seen["zero_matrix"]
    assert Z.ntiles == 3 and Z.cw_max == 0 and Z.windowed == 0 and Z.c16back == 0 and Z.col16 is not None and not Z.col16.any()


@pytest.mark.parametrize("long", [2048, 2049])
def test_row_at_the_nonzero_limit(built, long):
    lens = [3, 5, long, 0, 2, 7]
    rp, ci, va = _from_lens(lens, 2100, seed=long)
    P = check(CC.tile_plan(checkers.load_hostcheck(), rp, ci, va), rp, ci, va)
    # the row starts a tile; with exactly 2 048 entries the empty row behind it still fits, with 2 049 the tile is the row alone
    assert P.tiles.tolist() == ([0, 2, 4, 6] if long == 2048 else [0, 2, 3, 6])


@pytest.mark.parametrize("nrows", [256, 257])
def test_row_limit(built, nrows):
    rp, ci, va = _from_lens([1] * nrows, nrows, cols=lambda i, l: np.array([i]))
    P = check(CC.tile_plan(checkers.load_hostcheck(), rp, ci, va), rp, ci, va)
    assert P.tiles.tolist() == ([0, 256] if nrows == 256 else [0, 256, 257])


@pytest.mark.parametrize("width", [3072, 3073])
def test_window_limit(built, width):
    n = 4000
    rp, ci, va = _from_lens([2] + [1] * (n - 1), n, cols=lambda i, l: np.array([0, width - 1]) if i == 0 else np.array([min(i, width - 1)]))
    P = check(CC.tile_plan(checkers.load_hostcheck(), rp, ci, va), rp, ci, va)
    assert tuple(P.win[0]) == ((0, 3072) if width == 3072 else (0, 0))
    assert P.cw_max == (3072 if width == 3072 else 256)


@pytest.mark.parametrize("reach", [65535, 65536])
def test_reach_of_the_16_bit_stream(built, reach):
    n = reach + 1
    rp, ci, va = _from_lens([2] + [0] * 299, n, cols=lambda i, l: np.array([0, reach])[:l])
    P = check(CC.tile_plan(checkers.load_hostcheck(), rp, ci, va, xlen=n, ncols_global=n), rp, ci, va, xlen=n, ncols_global=n)
    assert (P.col16 is not None) == (reach == 65535)
    if reach == 65535: assert P.col16[1] == 65535
    # complex values never get the stream
    Pz = check(CC.tile_plan(checkers.load_hostcheck(), rp, ci, va.astype(np.complex128), xlen=n, ncols_global=n, real=False), rp, ci,
               va.astype(np.complex128), xlen=n, ncols_global=n, real=False)
    assert Pz.col16 is None and Pz.c16back == 0


def test_row_slab_with_halo(built):
    """rows [1000, 1800) of a band matrix of 3 000 rows, half-width 100: columns on both sides of the slab"""
    n, row0, m = 3000, 1000, 800
    rng = np.random.default_rng(4)
    cols = lambda i, l: np.unique(np.concatenate([[row0 + i - 100, row0 + i, row0 + i + 100], rng.integers(row0 + i - 100, row0 + i + 101, size=12)]))
    rows = [cols(i, 0) for i in range(m)]
    rp = np.zeros(m + 1, dtype=np.int32); rp[1:] = np.cumsum([len(r) for r in rows])
    ci = np.concatenate(rows).astype(np.int32)
    va = rng.standard_normal(len(ci))
    va[ci == row0 + np.repeat(np.arange(m), np.diff(rp))] = 1000.0 + np.arange(m)         # the diagonal, recognisable
    P = check(CC.tile_plan(checkers.load_hostcheck(), rp, ci, va, row0=row0, ncols_global=n), rp, ci, va, row0=row0, ncols_global=n)
    assert (P.halo_lo, P.halo_hi) == (100, 100) and P.windowed == 0
    assert np.array_equal(P.diag, 1000.0 + np.arange(m))                                    # taken at column row0 + i
    # no tile is windowable across the slab edge; the ones in between are
    assert tuple(P.win[0]) == (0, 0) and tuple(P.win[P.ntiles - 1]) == (0, 0)
    inner = [k for k in range(P.ntiles) if P.win[k, 1] > 0]
    assert inner and all(P.win[k, 0] >= row0 and P.win[k, 0] + P.win[k, 1] <= row0 + m for k in inner)
    assert P.col16 is not None and P.c16back == 100


def test_rectangular(built):
    """hipk_csr_create_rect's call: row0 = x0 = 0, every input entry owned"""
    m, n = 500, 1200
    rng = np.random.default_rng(6)
    lens = rng.integers(0, 12, size=m)
    rp, ci, va = _from_lens(lens, n, cols=lambda i, l: np.sort(rng.choice(n, size=l, replace=False)))
    P = check(CC.tile_plan(checkers.load_hostcheck(), rp, ci, va, xlen=n, ncols_global=n), rp, ci, va, xlen=n, ncols_global=n)
    assert (P.halo_lo, P.halo_hi) == (0, 0) and P.cw_max > 0 and P.windowed == 0
