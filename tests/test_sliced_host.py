"""The host converter of the sliced-ELL form (csrc/csr_tools.c: primme_amd_csr_to_sliced, layout in include/primme_amd_io.h),
through the CPU checker library as tests/test_ingest.py calls the ingest: expanding the sliced arrays gives the CSR arrays back
bit for bit; perm is a permutation inside every window; lengths never grow inside a window; the padding is the one numpy
computes; 16-bit indices for the LUNDA tiling, 32-bit for a slice that spans 70 000 columns; the fallback by padding."""
import numpy as np
import pytest

import checkers
import sliced_cases as SC


def expand(S):
    """the CSR arrays from the sliced ones, reading exactly the entries the layout promises"""
    m = S.m
    rows = [None] * m
    for p in range(m):
        s, l, w0 = p // 64, p % 64, (p // 256) * 256
        q = S.base[s] + 64 * np.arange(S.len[p]) + l
        assert np.all(q < S.base[s + 1])
        rows[w0 + int(S.perm[p])] = (S.idx[q].astype(np.int64) + S.cmin[s], S.val[q])
    assert all(r is not None for r in rows)              # every row has a slot
    rp = np.zeros(m + 1, dtype=np.int64); rp[1:] = np.cumsum([len(c) for c, _ in rows])
    return rp.astype(np.int32), np.concatenate([c for c, _ in rows]).astype(np.int32), np.concatenate([v for _, v in rows])


def check(S, rp, ci, va):
    m, nnz = len(rp) - 1, len(ci)
    assert (S.m, S.nnz, S.nslices) == (m, nnz, (m + 63) // 64)
    padded, slen, perm = SC.padding_numpy(rp)
    # perm: a permutation inside every window, THE stable descending one; lengths non-increasing inside a window
    for w0 in range(0, m, 256):
        nr = min(256, m - w0)
        assert sorted(S.perm[w0:w0 + nr].tolist()) == list(range(nr))
        assert np.all(np.diff(S.len[w0:w0 + nr].astype(np.int64)) <= 0)
    assert np.array_equal(S.perm[:m], perm) and np.array_equal(S.len[:m], slen)
    assert not S.len[m:].any()                           # the slots of the ragged last slice that do not exist
    # widths and padding
    width = np.diff(S.base) // 64
    assert S.base[0] == 0 and np.all(np.diff(S.base) % 64 == 0) and S.base.dtype == np.int64
    assert np.array_equal(width, [S.len[64 * s] for s in range(S.nslices)])
    assert S.padded == padded and S.padded >= nnz
    # the arrays give the matrix back: values bit for bit, columns and order inside the rows
    r2, c2, v2 = expand(S)
    assert np.array_equal(r2, rp) and np.array_equal(c2, ci)
    assert v2.dtype == va.dtype and v2.tobytes() == np.ascontiguousarray(va).tobytes()
    # padding: value 0 and a column inside the matrix
    live = np.zeros(int(S.base[-1]), dtype=bool)
    for p in range(m):
        live[S.base[p // 64] + 64 * np.arange(S.len[p]) + p % 64] = True
    assert not S.val[~live].any()
    col = S.idx.astype(np.int64) + np.repeat(S.cmin, np.diff(S.base))
    assert np.all((col >= 0) & (col <= ci.max()))
    # one index width per matrix, 16 bits exactly when every slice spans fewer than 65 536 columns
    span = 0
    for s in range(S.nslices):
        c = col[S.base[s]:S.base[s + 1]][live[S.base[s]:S.base[s + 1]]]
        if len(c): span = max(span, int(c.max() - c.min()))
    assert bool(S.idx16) == (span < 65536) and S.idx.dtype == (np.uint16 if S.idx16 else np.int32)
    if not S.idx16: assert not S.cmin.any()


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("name", SC.SHAPES + ["random_band", "holes257"])
def test_round_trip(built, name, dtype):
    lib = checkers.load_hostcheck()
    rp, ci, va = SC.matrix(name)
    va = va.astype(dtype)
    rc, S = SC.to_sliced(lib, rp, ci, va, max_padding=1e30)         # every shape, whatever its padding
    assert rc == 0
    check(S, rp, ci, va)
    if name != "band1": assert S.idx16 == 1
    # under the device operator's limit the same form or the fallback, by the ratio numpy computes
    ratio = SC.padding_numpy(rp)[0] / len(ci)
    rc2, S2 = SC.to_sliced(lib, rp, ci, va)
    assert (rc2 == 0) == (ratio <= SC.MAX_PADDING), (name, ratio)
    if S2 is not None: assert S2.padded == S.padded and np.array_equal(S2.idx, S.idx)
    print(f"{name}: padded / nnz = {ratio:.4f}")


def test_shapes_under_the_limit(built):
    """the shapes the device tests run take the form, not the fallback"""
    for name in SC.SHAPES + ["random_band", "holes257", "wide", "lunda4"]:
        rp, ci, _ = SC.matrix(name)
        assert SC.padding_numpy(rp)[0] <= SC.MAX_PADDING * len(ci), name


def test_empty_slice_and_empty_rows(built):
    rp, ci, va = SC.matrix("empty_rows")
    rc, S = SC.to_sliced(checkers.load_hostcheck(), rp, ci, va)
    assert rc == 0
    assert S.base[4] == S.base[3] and not S.len[192:256].any()      # slice 3: 64 empty rows, width 0
    assert sorted(S.perm[176:256].tolist()) == list(range(100, 180))


def test_lunda_tiling_takes_16_bit_indices(built):
    rp, ci, va = SC.matrix("lunda3")
    assert len(rp) - 1 == 441
    rc, S = SC.to_sliced(checkers.load_hostcheck(), rp, ci, va)
    assert rc == 0 and S.idx16 == 1 and S.idx.dtype == np.uint16
    assert S.padded / S.nnz <= 1.15                                  # sorted inside 256 rows; unsorted slices of 64 pad by a quarter


def test_wide_slice_takes_32_bit_indices(built):
    rp, ci, va = SC.matrix("wide")
    assert len(rp) - 1 == 70000 and ci[rp[1] - 1] == 69999
    rc, S = SC.to_sliced(checkers.load_hostcheck(), rp, ci, va)
    assert rc == 0 and S.idx16 == 0
    check(S, rp, ci, va)


def test_fallback_by_padding(built):
    rp, ci, va = SC.matrix("fallback300")
    assert len(rp) - 1 == 300 and np.diff(rp).max() == 250 and np.sum(np.diff(rp) == 3) == 299
    lib = checkers.load_hostcheck()
    assert SC.padding_numpy(rp)[0] > SC.MAX_PADDING * len(ci)
    assert SC.to_sliced(lib, rp, ci, va) == (1, None)
    # the limit is a parameter: just above this matrix' ratio the form is built
    padded = SC.padding_numpy(rp)[0]
    rc, S = SC.to_sliced(lib, rp, ci, va, max_padding=padded / len(ci) * (1 + 1e-12))
    assert rc == 0 and S.padded == padded
    # an empty matrix has nothing to slice
    assert SC.to_sliced(lib, np.zeros(5, dtype=np.int32), np.zeros(0, dtype=np.int32), np.zeros(0))[0] == 1
