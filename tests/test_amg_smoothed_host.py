"""The host side of smoothed aggregation, without a GPU: primme_amd_amg_plan_create_smoothed (csrc/csr_tools.c) through the CPU
checker library, on the matrices of amg_cases.matrices().  P_l against the dense (I - (omega / rho) D^-1 M) T, R_l its bitwise
transpose, the constant reproduced where M 1 vanishes, the coarse matrices against the dense P' M P and exactly symmetric, the
aggregates of level 0 those of the plain plan, determinism, the plain plan untouched, the error returns, and the V-cycle of the
restatement (tests/amg_smoothed_cases.py): K symmetric to 1e-13 |K| and positive definite, cond(K M) below that of plain
aggregation on 33 x 35 and 65 x 67 and growing less between them.

cond(K M) on 65 x 67 (4355 rows) comes from 120 Lanczos steps with full reorthogonalisation for K M in the M inner product,
where it is self-adjoint: the ratio of the extreme Ritz values, a lower bound of cond(K M) that is tight once they have
converged.  On 33 x 35 the same estimate is checked against the eigenvalues of the dense K M to 1e-6; the inequalities asserted
have margins of tens of per cent.  The values printed:
plain 3.146 -> 9.520, smoothed 1.238 -> 1.507."""
import math

import numpy as np
import pytest

import amg_cases as AMG
import amg_smoothed_cases as SA
import checkers
from primme_amd import problems

_mats = AMG.matrices()
_plans = {}
EPS = 2.0 ** -52


def _plan(name, shift=0.0):
    if (name, shift) not in _plans:
        rc, lv, om = SA.c_plan(checkers.load_hostcheck(), *_mats[name], shift=shift)
        assert rc == 0 and om == SA.OMEGA
        _plans[(name, shift)] = lv
    return _plans[(name, shift)]


def _same(a, b):
    assert len(a) == len(b)
    for x, y in zip(a, b):
        assert x.keys() == y.keys()
        for k in x:
            assert np.array_equal(x[k], y[k]), k


@pytest.mark.parametrize("name", list(_mats))
def test_plan(built, name):
    rp, ci, va = _mats[name]
    lib = checkers.load_hostcheck()
    lv = _plan(name)
    rc, plain = AMG.c_plan(lib, rp, ci, va)
    assert rc == 0
    # level 0 is the matrix, and its aggregates are those of the plain plan
    for k in ("n", "nnz", "nc", "rho", "rowptr", "colind", "values", "dinv") + (("agg", "aggptr", "aggrows") if plain[0]["nc"] else ()):
        assert np.array_equal(lv[0][k], plain[0][k]), k
    assert (len(lv) == 1) == (len(plain) == 1)
    for l, v in enumerate(lv):
        n = v["n"]
        M = AMG.dense(n, v["rowptr"], v["colind"], v["values"])
        assert np.array_equal(M, M.T)
        assert np.array_equal(v["dinv"], 1.0 / np.diag(M))
        bound = np.max(np.abs(M).sum(axis=1) / np.diag(M))
        assert abs(v["rho"] - bound) <= 1e-14 * bound
        for i in range(n):
            assert np.all(np.diff(v["colind"][v["rowptr"][i]:v["rowptr"][i + 1]]) > 0)
        if l == len(lv) - 1:
            assert v["nc"] == 0 and "transfer_null" in v
            continue
        nc = v["nc"]
        assert n > AMG.DENSE_ROWS and nc <= 0.8 * n and lv[l + 1]["n"] == nc and "transfer_null" not in v
        assert np.array_equal(np.sort(v["aggrows"]), np.arange(n)) and v["aggptr"][-1] == n
        # P = (I - (omega / rho) D^-1 M) T, columns sorted, one entry per position
        assert v["prowptr"][0] == 0 and v["prowptr"][-1] == v["pnnz"] == len(v["pcolind"])
        for i in range(n):
            assert np.all(np.diff(v["pcolind"][v["prowptr"][i]:v["prowptr"][i + 1]]) > 0)
        assert v["pcolind"].min() >= 0 and v["pcolind"].max() < nc
        P = SA.dense_rect(n, nc, v["prowptr"], v["pcolind"], v["pvalues"])
        T = AMG.prolongation(v["agg"], nc)
        ref = (np.eye(n) - (SA.OMEGA / v["rho"]) * v["dinv"][:, None] * M) @ T
        assert np.abs(P - ref).max() <= 1e-14 * np.abs(P).max()
        # R is the transpose, bit for bit, with ascending columns
        assert v["rrowptr"][0] == 0 and v["rrowptr"][-1] == v["pnnz"]
        for j in range(nc):
            assert np.all(np.diff(v["rcolind"][v["rrowptr"][j]:v["rrowptr"][j + 1]]) > 0)
        prow = np.repeat(np.arange(n), np.diff(v["prowptr"]))
        rrow = np.repeat(np.arange(nc), np.diff(v["rrowptr"]))
        order = np.lexsort((prow, v["pcolind"]))                      # the entries of P by column, then row
        assert np.array_equal(v["pcolind"][order], rrow) and np.array_equal(prow[order], v["rcolind"])
        assert np.array_equal(v["pvalues"][order].view(np.int64), v["rvalues"].view(np.int64))
        # the coarse matrix
        c = lv[l + 1]
        Mc = AMG.dense(c["n"], c["rowptr"], c["colind"], c["values"])
        assert np.abs(Mc - P.T @ M @ P).max() <= 1e-13 * np.linalg.norm(M, 2)
    print(f"{name}: levels {[v['n'] for v in lv]} (plain {[v['n'] for v in plain]}), operator complexity "
          f"{sum(v['nnz'] for v in lv) / lv[0]['nnz']:.3f} (plain {sum(v['nnz'] for v in plain) / plain[0]['nnz']:.3f}), "
          f"entries per row of P {[round(v['pnnz'] / v['n'], 2) for v in lv[:-1]]}, longest row of P' "
          f"{[int(np.diff(v['rrowptr']).max()) for v in lv[:-1]]}")
    # two calls give identical plans
    rc, again, _ = SA.c_plan(lib, rp, ci, va)
    assert rc == 0
    _same(lv, again)
    # the plain plan: no transfer matrices, omega 0, and the level data amg_cases reads
    rc, p2, om = SA.c_plan(lib, rp, ci, va, omega=None)
    assert rc == 0 and om == 0.0 and all("transfer_null" in v for v in p2)
    for v in p2:
        del v["transfer_null"]
    _same(p2, plain)


def test_expected_shapes(built):
    assert [v["n"] for v in _plan("lap_33x35")] == [1155, 206]
    assert len(_plan("lunda_x4")) == 2 and _plan("lunda_x4")[0]["n"] == 588
    assert [v["n"] for v in _plan("diag_300")] == [300] and len(_plan("lap_6x7")) == 1


@pytest.mark.parametrize("name,dims", [("lap_33x35", (33, 35))])
def test_constant_is_reproduced(built, name, dims):
    """rows i with (M 1)_i = 0, the interior of the grid: row i of P_0 sums to 1"""
    rp, ci, va = _mats[name]
    v = _plan(name)[0]
    rowsum = np.add.reduceat(va, rp[:-1])
    interior = np.flatnonzero(rowsum == 0.0)
    assert len(interior) == (dims[0] - 2) * (dims[1] - 2)
    worst = 0.0
    for i in interior:
        s = math.fsum(v["pvalues"][v["prowptr"][i]:v["prowptr"][i + 1]])
        worst = max(worst, abs(s - 1.0))
    print(f"{name}: {len(interior)} interior rows, largest |sum_j p_ij - 1| = {worst / EPS:.2f} eps")
    assert worst <= 4 * EPS
    # and so P_0 1_c = 1 there: the constant on the coarse level is the constant on the fine one
    P = SA.dense_rect(v["n"], v["nc"], v["prowptr"], v["pcolind"], v["pvalues"])
    assert np.abs((P @ np.ones(v["nc"]))[interior] - 1.0).max() <= 4 * EPS


def test_3d_constant_is_reproduced(built):
    rp, ci, va, _ = problems.laplacian_csr((9, 8, 7))
    rc, lv, _ = SA.c_plan(checkers.load_hostcheck(), rp, ci, va)
    assert rc == 0 and len(lv) >= 2
    v = lv[0]
    interior = np.flatnonzero(np.add.reduceat(va, rp[:-1]) == 0.0)
    assert len(interior) == 7 * 6 * 5
    worst = max(abs(math.fsum(v["pvalues"][v["prowptr"][i]:v["prowptr"][i + 1]]) - 1.0) for i in interior)
    assert worst <= 4 * EPS


def test_float_values_and_shift(built):
    rp, ci, va = _mats["lap_33x35"]
    rc, f, _ = SA.c_plan(checkers.load_hostcheck(), rp, ci, va.astype(np.float32), shift=0.5)
    assert rc == 0
    _same(f, _plan("lap_33x35", 0.5))                                 # 4, -1 and 0.5 are floats


def test_error_returns(built):
    lib = checkers.load_hostcheck()
    rp, ci, va = _mats["lap1d_5"]
    for omega in (0.0, 2.0, -1.0, float("nan"), 2.5):
        assert SA.c_plan(lib, rp, ci, va, omega=omega)[0] == -1
    assert SA.c_plan(lib, rp, ci, va, omega=1e-3)[0] == 0 and SA.c_plan(lib, rp, ci, va, omega=1.999)[0] == 0
    # the plain plan's cases, through both functions
    for omega in (SA.OMEGA, None):
        assert SA.c_plan(lib, rp[:1], ci[:0], va[:0], omega=omega)[0] == -1                  # n = 0
        keep = ci != np.repeat(np.arange(5), np.diff(rp))
        keep[0] = True
        rp2 = np.concatenate([[0], np.cumsum([keep[rp[i]:rp[i + 1]].sum() for i in range(5)])])
        assert SA.c_plan(lib, rp2, ci[keep], va[keep], omega=omega)[0] == -1                 # rows without a diagonal entry
        for bad in (0.0, -2.0):
            vb = va.copy()
            vb[np.flatnonzero(ci == np.repeat(np.arange(5), np.diff(rp)))[3]] = bad
            assert SA.c_plan(lib, rp, ci, vb, omega=omega)[0] == -1                          # m_ii <= 0
        assert SA.c_plan(lib, rp, ci, va, shift=-1.0, omega=omega)[0] == -1
        assert SA.c_plan(lib, rp, ci, va, theta=1.0, omega=omega)[0] == -1 and SA.c_plan(lib, rp, ci, va, theta=-0.1, omega=omega)[0] == -1


@pytest.mark.parametrize("shift", [0.0, 0.5])
@pytest.mark.parametrize("name", ["lap1d_5", "lap_6x7", "lap_33x35", "lap_5x4x3"])
def test_vcycle_is_symmetric_positive_definite(built, name, shift):
    lv = _plan(name, shift)
    H = SA.Hierarchy(lv)
    K = H.matrix()
    assert np.abs(K - K.T).max() <= 1e-13 * np.linalg.norm(K, 2)
    ev = np.linalg.eigvalsh(0.5 * (K + K.T))
    assert ev.min() > 0.0
    km = np.linalg.eigvals(K @ H.M[0]).real
    print(f"{name} shift {shift}: levels {[v['n'] for v in lv]}, eig(K) in [{ev.min():.3e}, {ev.max():.3e}], "
          f"cond(K M) = {km.max() / km.min():.3f}")


def _cond_lanczos(H, steps=120):
    """cond(K M) from the extreme Ritz values of `steps` Lanczos steps for K M, self-adjoint in the M inner product"""
    M = H.M[0]
    n = M.shape[0]
    q = np.random.default_rng(n).standard_normal((n, 1))
    Q, MQ = np.zeros((n, 0)), np.zeros((n, 0))
    Tm = np.zeros((steps, steps))
    for k in range(steps):
        for _ in range(2):
            q = q - Q @ (MQ.T @ q)
        mq = M @ q
        nrm = float(np.sqrt((q * mq).sum()))
        q, mq = q / nrm, mq / nrm
        Q, MQ = np.hstack([Q, q]), np.hstack([MQ, mq])
        q = H.vcycle(mq)
        Tm[:k + 1, k] = (MQ.T @ q)[:, 0]
    ev = np.linalg.eigvalsh(np.triu(Tm) + np.triu(Tm, 1).T)          # column k holds rows 0 .. k
    return ev.max() / ev.min()


def test_condition_numbers_against_plain_aggregation(built):
    lib = checkers.load_hostcheck()
    cond = {}
    for dims in ((33, 35), (65, 67)):
        rp, ci, va, _ = problems.laplacian_csr(dims)
        rc, plain = AMG.c_plan(lib, rp, ci, va)
        assert rc == 0
        rc, smooth, _ = SA.c_plan(lib, rp, ci, va)
        assert rc == 0
        Hp, Hs = AMG.Hierarchy(plain), SA.Hierarchy(smooth)
        cond[dims] = (_cond_lanczos(Hp), _cond_lanczos(Hs))
        if dims == (33, 35):                                          # the estimate against the dense K M
            for H, c in zip((Hp, Hs), cond[dims]):
                km = np.linalg.eigvals(H.matrix() @ H.M[0]).real
                assert abs(c - km.max() / km.min()) <= 1e-6 * c
        cx = [sum(v["nnz"] for v in lv) / lv[0]["nnz"] for lv in (plain, smooth)]
        print(f"{dims[0]} x {dims[1]}: plain levels {[v['n'] for v in plain]} complexity {cx[0]:.3f} cond(K M) = {cond[dims][0]:.3f}; "
              f"smoothed levels {[v['n'] for v in smooth]} complexity {cx[1]:.3f} cond(K M) = {cond[dims][1]:.3f}")
        assert cond[dims][1] < cond[dims][0]
    gp, gs = (cond[(65, 67)][k] / cond[(33, 35)][k] for k in (0, 1))
    print(f"growth of cond(K M) from 33 x 35 to 65 x 67: plain {gp:.2f} x, smoothed {gs:.2f} x")
    assert gs < gp
