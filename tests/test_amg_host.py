"""The host side of the aggregation algebraic multigrid preconditioner, without a GPU: primme_amd_amg_plan_create and
primme_amd_amg_coarse_inverse (csrc/csr_tools.c) through the CPU checker library.  The invariants of the plan on ten matrices
(every row in one aggregate, the inverse map, Galerkin matrices against the dense P' M P, symmetry, rho as a bound, the stop
rule, the three passes against a restatement in Python, determinism), the error returns, and the properties of the V-cycle the
device code implements on the dense restatement of tests/amg_cases.py: K symmetric to 1e-13 |K|, every eigenvalue positive.
The condition numbers it prints are the ones in DESIGN.md section 4o."""
import numpy as np
import pytest

import amg_cases as AMG
import checkers

_mats = AMG.matrices()
_plans = {}


def _plan(name, shift=0.0):
    if (name, shift) not in _plans:
        rc, lv = AMG.c_plan(checkers.load_hostcheck(), *_mats[name], shift=shift)
        assert rc == 0
        _plans[(name, shift)] = lv
    return _plans[(name, shift)]


def _aggregate(n, rp, ci, va, theta):
    """the three passes of primme_amd_io.h, restated: (agg, number of aggregates)"""
    dg = np.zeros(n)
    rows = np.repeat(np.arange(n), np.diff(rp))
    np.add.at(dg, rows[ci == rows], va[ci == rows])
    strong = [[(int(ci[q]), abs(va[q])) for q in range(rp[i], rp[i + 1])
               if ci[q] != i and abs(va[q]) >= theta * np.sqrt(dg[i] * dg[ci[q]])] for i in range(n)]
    agg = [-1] * n
    nc = 0
    for i in range(n):
        if agg[i] < 0 and all(agg[j] < 0 for j, _ in strong[i]):
            agg[i] = nc
            for j, _ in strong[i]: agg[j] = nc
            nc += 1
    first = list(agg)
    for i in range(n):
        if first[i] < 0:
            cand = [(-v, first[j]) for j, v in strong[i] if first[j] >= 0]
            if cand: agg[i] = min(cand)[1]
    for i in range(n):
        if agg[i] < 0:
            agg[i] = nc
            for j, _ in strong[i]:
                if agg[j] < 0: agg[j] = nc
            nc += 1
    return np.array(agg), nc


@pytest.mark.parametrize("name", list(_mats))
def test_plan_invariants(built, name):
    rp, ci, va = _mats[name]
    lv = _plan(name)
    assert 1 <= len(lv) <= AMG.MAXLEVELS and lv[0]["n"] == len(rp) - 1
    assert np.array_equal(AMG.dense(lv[0]["n"], lv[0]["rowptr"], lv[0]["colind"], lv[0]["values"]), AMG.dense(len(rp) - 1, rp, ci, va))
    for l, v in enumerate(lv):
        n = v["n"]
        M = AMG.dense(n, v["rowptr"], v["colind"], v["values"])
        assert np.array_equal(M, M.T)
        assert np.array_equal(v["dinv"], 1.0 / np.diag(M))
        bound = np.max(np.abs(M).sum(axis=1) / np.diag(M))
        assert abs(v["rho"] - bound) <= 1e-14 * bound
        d = np.sqrt(v["dinv"])
        assert np.linalg.eigvalsh(d[:, None] * M * d[None, :]).max() <= v["rho"] * (1 + 1e-14)
        last = l == len(lv) - 1
        if n > 1 or not last:
            agg, nc = _aggregate(n, v["rowptr"], v["colind"], v["values"], 0.08)
        if last:
            # the stop rule: small enough, the level cap, or an aggregation that keeps more than 0.8 of the rows
            assert v["nc"] == 0 and (n <= AMG.DENSE_ROWS or len(lv) == AMG.MAXLEVELS or nc > 0.8 * n)
            continue
        assert n > AMG.DENSE_ROWS and v["nc"] <= 0.8 * n and lv[l + 1]["n"] == v["nc"]
        assert np.array_equal(v["agg"], agg) and v["nc"] == nc
        # every row in exactly one aggregate, every aggregate inhabited; aggptr / aggrows invert agg with ascending rows
        assert v["agg"].min() == 0 and v["agg"].max() == nc - 1 and len(np.unique(v["agg"])) == nc
        assert v["aggptr"][0] == 0 and v["aggptr"][-1] == n and np.all(np.diff(v["aggptr"]) >= 1)
        assert np.array_equal(np.sort(v["aggrows"]), np.arange(n))
        for j in range(nc):
            r = v["aggrows"][v["aggptr"][j]:v["aggptr"][j + 1]]
            assert np.all(np.diff(r) > 0) and np.all(v["agg"][r] == j)
        # Galerkin: sorted columns, one entry per position, P' M P
        c = lv[l + 1]
        for i in range(c["n"]):
            assert np.all(np.diff(c["colind"][c["rowptr"][i]:c["rowptr"][i + 1]]) > 0)
        P = AMG.prolongation(v["agg"], nc)
        Mc = AMG.dense(c["n"], c["rowptr"], c["colind"], c["values"])
        assert np.abs(Mc - P.T @ M @ P).max() <= 1e-14 * np.linalg.norm(M, 2)
    sizes = [v["n"] for v in lv]
    print(f"{name}: levels {sizes}, operator complexity {sum(v['nnz'] for v in lv) / lv[0]['nnz']:.3f}, rho {[round(v['rho'], 3) for v in lv]}")
    # two calls give identical plans
    rc, again = AMG.c_plan(checkers.load_hostcheck(), rp, ci, va)
    assert rc == 0 and len(again) == len(lv)
    for a, b in zip(lv, again):
        assert a.keys() == b.keys()
        for k in a:
            assert np.array_equal(a[k], b[k]), k


def test_expected_shapes(built):
    """what the issue says of three of the matrices"""
    assert [v["n"] for v in _plan("diag_300")] == [300]                     # stalls at level 0: the Chebyshev last level
    assert "G" not in _plan("diag_300")[0]
    assert len(_plan("lap_33x35")) >= 2 and _plan("lap_33x35")[-1]["n"] <= AMG.DENSE_ROWS
    assert [v["n"] for v in _plan("lunda")] == [147] and len(_plan("lunda_x4")) >= 2
    one = _plan("lap1d_1")
    assert len(one) == 1 and one[0]["G_rc"] == 0 and abs(one[0]["G"][0, 0] - 0.5) <= 2.0 ** -52


def test_float_values_and_shift(built):
    rp, ci, va = _mats["lap_33x35"]
    lib = checkers.load_hostcheck()
    rc, f = AMG.c_plan(lib, rp, ci, va.astype(np.float32), shift=0.5)
    assert rc == 0
    d = _plan("lap_33x35", 0.5)
    M0 = AMG.dense(d[0]["n"], d[0]["rowptr"], d[0]["colind"], d[0]["values"])
    assert np.array_equal(M0, AMG.dense(len(rp) - 1, rp, ci, va) + 0.5 * np.eye(len(rp) - 1))
    assert len(f) == len(d) and all(np.array_equal(a["values"], b["values"]) for a, b in zip(f, d))    # 4, -1 and 0.5 are floats


def test_coarse_inverse(built):
    for name in ("lap_6x7", "lunda", "lap_33x35", "lunda_x4"):
        v = _plan(name)[-1]
        M = AMG.dense(v["n"], v["rowptr"], v["colind"], v["values"])
        assert v["G_rc"] == 0 and np.array_equal(v["G"], v["G"].T)
        res = np.abs(v["G"] @ M - np.eye(v["n"])).max()
        print(f"{name}: last level {v['n']} rows, cond {np.linalg.cond(M):.3e}, |G M - I| = {res:.2e}")
        assert res <= 64 * 2.0 ** -52 * v["n"] * np.linalg.cond(M)
    # not positive definite: the factorisation fails
    rp, ci, va = np.array([0, 2, 4]), np.array([0, 1, 0, 1]), np.array([1.0, 2.0, 2.0, 1.0])
    rc, lv = AMG.c_plan(checkers.load_hostcheck(), rp, ci, va)
    assert rc == 0 and lv[0]["G_rc"] == -1


def test_plan_error_returns(built):
    lib = checkers.load_hostcheck()
    rp, ci, va = _mats["lap1d_5"]
    assert AMG.c_plan(lib, rp[:1], ci[:0], va[:0])[0] == -1                                  # n = 0
    keep = ci != np.repeat(np.arange(5), np.diff(rp))
    keep[0] = True                                                                           # row 0 keeps its diagonal
    rp2 = np.concatenate([[0], np.cumsum([keep[rp[i]:rp[i + 1]].sum() for i in range(5)])])
    assert AMG.c_plan(lib, rp2, ci[keep], va[keep])[0] == -1                                 # rows without a diagonal entry
    for bad in (0.0, -2.0):
        vb = va.copy()
        vb[np.flatnonzero(ci == np.repeat(np.arange(5), np.diff(rp)))[3]] = bad
        assert AMG.c_plan(lib, rp, ci, vb)[0] == -1                                          # m_ii <= 0
    assert AMG.c_plan(lib, rp, ci, va, shift=-1.0)[0] == -1 and AMG.c_plan(lib, rp, ci, va, theta=1.0)[0] == -1
    assert AMG.c_plan(lib, rp, ci, va, theta=-0.1)[0] == -1


@pytest.mark.parametrize("over", [1.0, 1.5])
@pytest.mark.parametrize("shift", [0.0, 0.5])
@pytest.mark.parametrize("name", ["lap1d_2", "lap1d_5", "lap_6x7", "lap_33x35", "lap_5x4x3"])
def test_vcycle_is_symmetric_positive_definite(built, name, shift, over):
    lv = _plan(name, shift)
    H = AMG.Hierarchy(lv, over=over)
    K = H.matrix()
    assert np.abs(K - K.T).max() <= 1e-13 * np.linalg.norm(K, 2)
    ev = np.linalg.eigvalsh(0.5 * (K + K.T))
    assert ev.min() > 0.0
    km = np.linalg.eigvals(K @ H.M[0]).real
    dm = H.dinv[0] * np.linalg.eigvalsh(H.M[0] * np.sqrt(H.dinv[0])[:, None] * np.sqrt(H.dinv[0])[None, :]) / H.dinv[0]
    print(f"{name} shift {shift} over {over}: levels {[v['n'] for v in lv]}, eig(K) in [{ev.min():.3e}, {ev.max():.3e}], "
          f"cond(K M) = {km.max() / km.min():.3f}, cond(D^-1 M) = {dm.max() / dm.min():.3f}")
