"""Helpers for the reusable hierarchy and the device set-up of smoothed aggregation (DESIGN.md section 4q;
csrc/hipk_amg_setup.hip, primme_amd_amg_hierarchy_create in csrc/amd_operator.hip): the matrices, and a numpy restatement of what
the device builds per level:

    P  by the definition of csrc/csr_tools.c: row i sums m_iq per aggregate in the row's order, p_iJ = [J = agg[i]] - c s_J with
       c = (omega / rho) dinv_i, the product and the difference rounded separately (numpy scalars do not contract)
    R  the stable transpose: the entries of P by column, then by row
    C  B = M P, the upper triangle of R B, mirrored; every entry carries the sum of the absolute values of its terms
       |r| |m| |p|, which is what the bound 32 eps sum|terms| of the kernel tests is made of
    dinv = 1 / diag, rho = max_i sum_j |m_ij| / m_ii

Everything is float64 and plain Python loops: the matrices have at most 4355 rows."""
import numpy as np

import amg_cases as AMG
from primme_amd import problems

EPS = 2.0 ** -52
OMEGAS = (4.0 / 3.0, 0.5)


def arrow(n=300):
    """dense first row and column: diagonal 300 there and 2 elsewhere, off-diagonals -1; row 0 has n entries"""
    rp, ci, va = [0], [], []
    for i in range(n):
        if i == 0:
            ci += list(range(n)); va += [300.0] + [-1.0] * (n - 1)
        else:
            ci += [0, i]; va += [-1.0, 2.0]
        rp.append(len(ci))
    return np.array(rp), np.array(ci), np.array(va)


def matrices():
    """name -> (rowptr, colind, values, shift, theta).  theta is 0.08 but for the arrow matrix, whose off-diagonal entries are
    weak at 0.08 (|m_0j| = 1 < 0.08 sqrt(600)): at 0.02 row 0 founds one aggregate of all 300 rows, R has one row of 300 entries"""
    out = {}
    for name, dims in (("lap1d_1", (1,)), ("lap1d_2", (2,)), ("lap_6x7", (6, 7)), ("lap_33x35", (33, 35)), ("lap_65x67", (65, 67)),
                       ("lap_9x8x7", (9, 8, 7))):
        out[name] = problems.laplacian_csr(dims)[:3] + (0.0, 0.08)
    out["lunda_x4"] = tuple(AMG.lunda_tiled(4)) + (0.0, 0.08)
    out["diag_300"] = (np.arange(301), np.arange(300), 1.0 + np.arange(300) / 7.0, 0.0, 0.08)
    out["arrow_300"] = arrow() + (0.0, 0.02)
    out["lap_33x35_shift"] = problems.laplacian_csr((33, 35))[:3] + (0.5, 0.08)
    return out


def custom_cases():
    """name -> (rowptr, colind, values, agg): aggregates of the test's own making for the matrices whose plan has one level, so
    that the kernels see them too: n = 1, n = 2, the diagonal matrix (rows without an off-diagonal entry) and the arrow matrix
    in pairs (row 0 of M has 300 entries in 150 aggregates: the long-row path of the prolongator and of M P)"""
    m = matrices()
    out = {"lap1d_1": m["lap1d_1"][:3] + (np.array([0]),), "lap1d_2": m["lap1d_2"][:3] + (np.array([0, 0]),),
           "lap1d_2_apart": m["lap1d_2"][:3] + (np.array([1, 0]),),
           "diag_300_pairs": m["diag_300"][:3] + (np.arange(300) // 2,),
           "arrow_300_pairs": m["arrow_300"][:3] + (np.arange(300) // 2,),
           "arrow_300_thirds": m["arrow_300"][:3] + ((np.arange(300) * 7) % 100,)}
    return out


def finish(rp, ci, va):
    n = len(rp) - 1
    dinv, rho = np.zeros(n), 0.0
    for i in range(n):
        d, s = 0.0, 0.0
        for q in range(rp[i], rp[i + 1]):
            if ci[q] == i:
                d += va[q]
            s += abs(va[q])
        dinv[i] = 1.0 / d
        rho = max(rho, s / d)
    return dinv, rho


def build_p(rp, ci, va, dinv, agg, w):
    n = len(rp) - 1
    prp, pci, pva = [0], [], []
    va = np.asarray(va, dtype=np.float64)
    for i in range(n):
        own = int(agg[i])
        acc = {own: np.float64(0.0)}
        for q in range(rp[i], rp[i + 1]):
            J = int(agg[ci[q]])
            acc[J] = acc[J] + va[q] if J in acc else va[q]
        c = np.float64(w) * np.float64(dinv[i])
        for J in sorted(acc):
            t = c * acc[J]                                            # rounded, then the difference rounded
            pci.append(J); pva.append(np.float64(1.0 if J == own else 0.0) - t)
        prp.append(len(pci))
    return np.array(prp, dtype=np.int64), np.array(pci, dtype=np.int64), np.array(pva, dtype=np.float64)


def transpose(n, nc, prp, pci, pva):
    prow = np.repeat(np.arange(n), np.diff(prp))
    order = np.lexsort((prow, pci))
    rrp = np.concatenate([[0], np.cumsum(np.bincount(pci, minlength=nc))]).astype(np.int64)
    return rrp, prow[order].astype(np.int64), pva[order]


def galerkin(M, P, R):
    """(crp, cci, cva, cmag): C = triu(R (M P)) mirrored, and sum |r| |m| |p| per entry"""
    (rp, ci, va), (prp, pci, pva), (rrp, rci, rva) = M, P, R
    n, nc = len(rp) - 1, len(rrp) - 1
    B = []
    for i in range(n):
        acc, mag = {}, {}
        for q in range(rp[i], rp[i + 1]):
            k, m = ci[q], va[q]
            for t in range(prp[k], prp[k + 1]):
                J = int(pci[t])
                acc[J] = acc.get(J, 0.0) + m * pva[t]
                mag[J] = mag.get(J, 0.0) + abs(m) * abs(pva[t])
        B.append((acc, mag))
    U = []
    for I in range(nc):
        acc, mag = {}, {}
        for a in range(rrp[I], rrp[I + 1]):
            bacc, bmag = B[rci[a]]
            r = rva[a]
            for J in bacc:
                if J >= I:
                    acc[J] = acc.get(J, 0.0) + r * bacc[J]
                    mag[J] = mag.get(J, 0.0) + abs(r) * bmag[J]
        U.append((acc, mag))
    rows = [dict() for _ in range(nc)]
    for I in range(nc):
        for J in U[I][0]:
            rows[I][J] = (U[I][0][J], U[I][1][J])
            rows[J][I] = (U[I][0][J], U[I][1][J])
    crp, cci, cva, cmag = [0], [], [], []
    for I in range(nc):
        for J in sorted(rows[I]):
            cci.append(J); cva.append(rows[I][J][0]); cmag.append(rows[I][J][1])
        crp.append(len(cci))
    return np.array(crp, dtype=np.int64), np.array(cci, dtype=np.int64), np.array(cva), np.array(cmag)


def level(rp, ci, va, dinv, rho, agg, nc, omega):
    """what the device builds from level l: P, R, C (with the magnitudes), dinv and rho of C"""
    n = len(rp) - 1
    P = build_p(rp, ci, va, dinv, agg, omega / rho)
    R = transpose(n, nc, *P)
    crp, cci, cva, cmag = galerkin((rp, ci, va), P, R)
    return dict(P=P, R=R, C=(crp, cci, cva), cmag=cmag)


def is_symmetric(crp, cci, cva):
    n = len(crp) - 1
    ent = {}
    for i in range(n):
        for q in range(crp[i], crp[i + 1]):
            ent[(i, int(cci[q]))] = cva[q]
    return all((j, i) in ent and np.float64(ent[(j, i)]).view(np.int64) == np.float64(v).view(np.int64) for (i, j), v in ent.items())


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.int64), b.view(np.int64))


def check_level(got, ref, host=None):
    """got / ref: dict(P, R, C) of a level, ref with cmag: indices equal, P and R the same bits, C within 32 eps sum|terms| and
    exactly symmetric.  host: the host plan's (P, R, C), compared in the same way.  Returns the largest fraction of the bound."""
    worst = 0.0
    for other in (ref,) + ((host,) if host is not None else ()):
        for k in ("P", "R", "C"):
            assert np.array_equal(got[k][0], other[k][0]) and np.array_equal(got[k][1], other[k][1]), k
        assert same_bits(got["P"][2], other["P"][2]) and same_bits(got["R"][2], other["R"][2])
        bound = 32 * EPS * ref["cmag"]
        frac = np.abs(np.asarray(got["C"][2]) - np.asarray(other["C"][2])) / np.maximum(bound, 1e-300)
        assert frac.max() <= 1.0, float(frac.max())
        worst = max(worst, float(frac.max()))
    assert is_symmetric(*got["C"])
    return worst


def host_level(v, nxt):
    """(P, R, C) of level v of a host plan (amg_smoothed_cases.c_plan), nxt the level after it"""
    return dict(P=(v["prowptr"], v["pcolind"], v["pvalues"]), R=(v["rrowptr"], v["rcolind"], v["rvalues"]),
                C=(nxt["rowptr"], nxt["colind"], nxt["values"]))
