"""The host scan of the diagonal-split row-pattern form (csrc/csr_tools.c: primme_amd_csr_row_patterns_diag), through the CPU
checker library: a row's pattern is its length, offsets, OFF-DIAGONAL values and the slot of its diagonal entry; the diagonal's
value is not in the table.  pid + table + diagonal must give the CSR arrays back, bit for bit."""
import ctypes as C

import numpy as np
import pytest

from primme_amd import problems
import checkers


def scan(rp, ci, va, row0=0):
    """-> None when the scan declines, else dict(pid, npat, ml, len, off, val, dslot)"""
    lib = checkers.load_hostcheck()
    rp = np.ascontiguousarray(rp, dtype=np.int32); ci = np.ascontiguousarray(ci, dtype=np.int32)
    va = np.ascontiguousarray(va)
    assert va.dtype in (np.float64, np.float32)
    m = len(rp) - 1
    pid, tlen, toff, tval, tds = (C.c_void_p() for _ in range(5))
    npat, ml = C.c_int(-7), C.c_int(-7)
    rc = lib.primme_amd_csr_row_patterns_diag(m, row0, rp.ctypes.data_as(C.c_void_p), ci.ctypes.data_as(C.c_void_p),
                                              va.ctypes.data_as(C.c_void_p), int(va.dtype == np.float32), C.byref(pid), C.byref(npat),
                                              C.byref(ml), C.byref(tlen), C.byref(toff), C.byref(tval), C.byref(tds))
    if rc == 1:
        assert not any(h.value for h in (pid, tlen, toff, tval, tds))       # nothing to release
        return None
    assert rc == 0

    def take(h, ctype, count):
        a = np.ctypeslib.as_array(C.cast(h, C.POINTER(ctype)), shape=(count,)).copy()
        lib.primme_amd_host_free(h)
        return a
    P, ML = npat.value, ml.value
    return dict(pid=take(pid, C.c_uint8, m + 1), npat=P, ml=ML, len=take(tlen, C.c_int32, P), off=take(toff, C.c_int32, P * ML).reshape(P, ML),
                val=take(tval, C.c_double, P * ML).reshape(P, ML), dslot=take(tds, C.c_int32, P))


def diagonal_of(rp, ci, va, row0):
    m = len(rp) - 1
    rows = np.repeat(np.arange(m), np.diff(rp))
    d = np.zeros(m, dtype=va.dtype)
    sel = ci == rows + row0
    d[rows[sel]] = va[sel]
    return d


def rebuild(t, diag, row0, dtype):
    """the CSR arrays from pid + table + diagonal"""
    pid = t["pid"][:-1].astype(np.int64)
    m = len(pid)
    lens = t["len"][pid]
    rp = np.zeros(m + 1, dtype=np.int64); np.cumsum(lens, out=rp[1:])
    slot = np.arange(t["ml"])[None, :]
    keep = slot < lens[:, None]
    col = (np.arange(m, dtype=np.int64)[:, None] + row0 + t["off"][pid])[keep]
    isd = (slot == t["dslot"][pid][:, None])
    val = np.where(isd, diag.astype(np.float64)[:, None], t["val"][pid])[keep]
    return rp.astype(np.int32), col.astype(np.int32), val.astype(dtype)


def check_table(t, rp, ci, va, row0):
    m = len(rp) - 1
    assert t["ml"] in (3, 5, 7, 8) and t["ml"] >= int(np.diff(rp).max()) and 1 <= t["npat"] <= 256
    assert t["pid"].shape == (m + 1,) and t["pid"][m] == 0 and t["pid"][:m].max() == t["npat"] - 1
    for p in range(t["npat"]):
        L, ds = t["len"][p], t["dslot"][p]
        zero = np.flatnonzero(t["off"][p, :L] == 0)
        assert (ds == -1 and len(zero) == 0) or (len(zero) == 1 and zero[0] == ds), (p, ds, zero)   # every dslot correct
        if ds >= 0: assert t["val"][p, ds] == 0.0                                                    # the value is NOT in the table
        assert not t["off"][p, L:].any() and not t["val"][p, L:].any()
    # no two patterns with the same key
    keys = {(t["len"][p], t["dslot"][p], t["off"][p].tobytes(), t["val"][p].tobytes()) for p in range(t["npat"])}
    assert len(keys) == t["npat"]
    r2, c2, v2 = rebuild(t, diagonal_of(rp, ci, va, row0), row0, va.dtype)
    assert np.array_equal(r2, rp) and np.array_equal(c2, ci)
    assert v2.dtype == va.dtype and v2.tobytes() == np.ascontiguousarray(va).tobytes()               # bitwise


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_schrodinger_patterns(built, dtype):
    """(a), (b): -Laplacian + random potential on 37 x 41 has the 9 patterns of the Laplacian"""
    rng = np.random.default_rng(5)
    dims = (37, 41)
    pot = rng.standard_normal(37 * 41) * 3.0
    rp, ci, va, n = problems.schrodinger_csr(dims, pot, dtype=dtype)
    lrp, lci, lva, _ = problems.laplacian_csr(dims, dtype=dtype)
    assert va.dtype == dtype and np.array_equal(rp, lrp) and np.array_equal(ci, lci)
    assert np.array_equal(diagonal_of(rp, ci, va, 0), (4.0 + pot).astype(dtype))
    t = scan(rp, ci, va)
    assert t is not None and t["npat"] == 9 and t["ml"] == 5
    assert np.all(t["dslot"] >= 0)
    check_table(t, rp, ci, va, 0)
    tl = scan(lrp, lci, lva)                      # the plain Laplacian: the same patterns, row by row
    assert tl["npat"] == 9 and np.array_equal(tl["pid"], t["pid"])
    # a callable potential gives the same matrix
    rp2, ci2, va2, _ = problems.schrodinger_csr(dims, lambda g: pot[g], dtype=dtype)
    assert np.array_equal(va2, va)


def test_absent_and_leading_diagonal(built):
    """(c): rows without a stored diagonal (dslot -1), and unsorted rows whose FIRST stored entry is the diagonal: order kept"""
    rng = np.random.default_rng(6)
    n = 1001
    rows, cols, vals = [], [], []
    for i in range(n):
        ent = [(i, 1.0 + rng.random())] if i % 3 else []          # every third row stores no diagonal
        for d, v in ((-7, 0.5), (2, -0.25), (-1, 1.5)):           # not in column order
            if 0 <= i + d < n: ent.append((i + d, v))
        for c, v in ent: rows.append(i); cols.append(c); vals.append(v)
    rp = np.zeros(n + 1, dtype=np.int64); np.add.at(rp, np.array(rows) + 1, 1); rp = np.cumsum(rp).astype(np.int32)
    ci = np.array(cols, dtype=np.int32); va = np.array(vals)
    t = scan(rp, ci, va)
    assert t is not None
    check_table(t, rp, ci, va, 0)
    pid = t["pid"][:-1]
    assert np.all(t["dslot"][pid[np.arange(n) % 3 == 0]] == -1)
    assert np.all(t["dslot"][pid[np.arange(n) % 3 != 0]] == 0)     # the diagonal is the first stored entry
    # interior rows: two patterns (with / without diagonal), each with the offsets in the stored order
    inner = t["off"][pid[500]], t["off"][pid[501]]
    assert list(inner[0][:4]) == [0, -7, 2, -1] or list(inner[0][:3]) == [-7, 2, -1]
    assert {tuple(inner[0][:t["len"][pid[500]]]), tuple(inner[1][:t["len"][pid[501]]])} <= {(0, -7, 2, -1), (-7, 2, -1)}


def test_declines(built):
    """(d): random off-diagonal values, a 9-entry row, a duplicated diagonal entry"""
    rng = np.random.default_rng(11)
    n = 5000                                                        # the `random` case of test_csr_row_pattern_form
    counts = rng.integers(1, 7, size=n)
    rp = np.zeros(n + 1, dtype=np.int64); np.cumsum(counts, out=rp[1:]); rp = rp.astype(np.int32)
    ci = np.concatenate([np.sort(rng.choice(n, size=c, replace=False)) for c in counts]).astype(np.int32)
    va = rng.standard_normal(len(ci))
    assert scan(rp, ci, va) is None
    # a Laplacian with one row of 9 entries
    rp, ci, va, n = problems.schrodinger_csr((64,), np.linspace(0.0, 1.0, 64))
    assert scan(rp, ci, va) is not None
    r = 30
    extra_c = np.array([2, 5, 8, 11, 40, 45], dtype=np.int32)
    ci9 = np.concatenate([ci[:rp[r]], extra_c[:3], ci[rp[r]:rp[r + 1]], extra_c[3:], ci[rp[r + 1]:]]).astype(np.int32)
    va9 = np.concatenate([va[:rp[r]], np.ones(3), va[rp[r]:rp[r + 1]], np.ones(3), va[rp[r + 1]:]])
    rp9 = rp.copy(); rp9[r + 1:] += 6
    assert rp9[r + 1] - rp9[r] == 9
    assert scan(rp9, ci9, va9) is None
    # the same row with 8 entries is accepted (the limit is 8, not fewer)
    ci8 = np.delete(ci9, rp9[r]); va8 = np.delete(va9, rp9[r]); rp8 = rp9.copy(); rp8[r + 1:] -= 1
    t = scan(rp8, ci8, va8)
    assert t is not None and t["ml"] == 8
    check_table(t, rp8, ci8, va8, 0)
    # a duplicated diagonal entry
    cid = np.insert(ci, rp[r + 1], r).astype(np.int32); vad = np.insert(va, rp[r + 1], 0.125); rpd = rp.copy(); rpd[r + 1:] += 1
    assert scan(rpd, cid, vad) is None


def test_slab_matches_whole(built):
    """(e): rows [2000, 5003) of the 23 x 19 x 17 grid as a slab: the patterns of those rows of the whole matrix"""
    dims = (23, 19, 17)
    n = int(np.prod(dims))
    pot = np.random.default_rng(8).standard_normal(n)
    row0, m = 2000, 3003
    rp, ci, va, _ = problems.schrodinger_csr(dims, pot, row0=row0, nrows=m)
    wrp, wci, wva, _ = problems.schrodinger_csr(dims, pot)
    ts, tw = scan(rp, ci, va, row0=row0), scan(wrp, wci, wva)
    assert ts is not None and tw is not None and tw["npat"] == 27
    check_table(ts, rp, ci, va, row0)
    check_table(tw, wrp, wci, wva, 0)
    for i in range(m):                                            # pattern numbers differ (order of first appearance), patterns do not
        p, q = ts["pid"][i], tw["pid"][row0 + i]
        assert ts["len"][p] == tw["len"][q] and ts["dslot"][p] == tw["dslot"][q]
        assert np.array_equal(ts["off"][p, :ts["len"][p]], tw["off"][q, :tw["len"][q]])
        assert np.array_equal(ts["val"][p, :ts["len"][p]], tw["val"][q, :tw["len"][q]])
    assert ts["npat"] == len(set(tw["pid"][row0:row0 + m].tolist()))
