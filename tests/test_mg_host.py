"""The host side of the geometric multigrid preconditioner, without a GPU: primme_amd_mg_plan (csrc/csr_tools.c) through the
CPU checker library against the numpy plan of tests/mg_cases.py, and the properties of the V-cycle the device code implements,
on that file's dense restatement: R = 2^-(coarsened dimensions) P', K symmetric to 1e-13 |K|, every eigenvalue of K positive.
The condition numbers of K M it prints are the ones in DESIGN.md section 4n."""
import numpy as np
import pytest

import checkers
import mg_cases as MG

PLAN_DIMS = [(1, 1, 1), (2, 2, 1), (5, 1, 1), (3, 3, 1), (6, 7, 1), (33, 35, 1), (9, 8, 7), (1000, 5, 1), (3162, 3163, 1),
             (125, 126, 127)]


@pytest.mark.parametrize("dims", PLAN_DIMS)
def test_plan_equals_numpy(built, dims):
    rc, n, w = MG.c_plan(checkers.load_hostcheck(), dims)
    assert rc == 0
    nn, ww = MG.plan(dims)
    assert n == nn and w == ww                      # the weights are powers of 4: exact
    # the rule itself, read off the result
    assert n[0] == tuple(dims) and w[0] == (1.0, 1.0, 1.0) and len(n) <= MG.MAXLEVELS
    for l in range(len(n) - 1):
        assert any(d >= 3 for d in n[l]) and np.prod(n[l]) > 32
        for d in range(3):
            assert (n[l + 1][d], w[l + 1][d]) == ((n[l][d] // 2, w[l][d] / 4) if n[l][d] >= 3 else (n[l][d], w[l][d]))
    assert not any(d >= 3 for d in n[-1]) or np.prod(n[-1]) <= 32 or len(n) == MG.MAXLEVELS


def test_plan_rejects_bad_dimensions(built):
    lib = checkers.load_hostcheck()
    assert MG.c_plan(lib, (0, 3, 1))[0] == -1 and MG.c_plan(lib, (4, -1, 1))[0] == -1
    assert MG.c_plan(lib, (65536, 65536, 1))[0] == -1          # more points than the kernels' 32-bit positions hold


def test_level_cap(built):
    """2^31 - 1 points in a row would need 26 halvings to reach 32 points: the plan stops at 24 levels"""
    rc, n, w = MG.c_plan(checkers.load_hostcheck(), (2 ** 31 - 1, 1, 1))
    assert rc == 0 and len(n) == MG.MAXLEVELS == 24 and n[-1] == ((2 ** 31 - 1) >> 23, 1, 1) and w[-1] == (4.0 ** -23, 1.0, 1.0)


@pytest.mark.parametrize("shift", [0.0, 0.5])
@pytest.mark.parametrize("dims", [(6, 7, 1), (5, 4, 3)])
def test_vcycle_is_symmetric_positive_definite(dims, shift):
    H = MG.Hierarchy(dims, shift=shift)
    assert H.L >= 1
    for l in range(H.L):
        nd = sum(MG.coarsened(H.n[l]))
        assert nd >= 1 and np.array_equal(H.R[l], 2.0 ** -nd * H.P[l].T)
    K = H.matrix()
    assert np.abs(K - K.T).max() <= 1e-13 * np.linalg.norm(K, 2)
    ev = np.linalg.eigvalsh(0.5 * (K + K.T))
    assert ev.min() > 0.0
    km = np.linalg.eigvals(K @ H.M[0]).real
    print(f"{dims} shift {shift}: levels {H.n}, eig(K) in [{ev.min():.3e}, {ev.max():.3e}], cond(K M) = {km.max() / km.min():.3f}")


def test_condition_number_at_33x35():
    """what DESIGN.md section 4n quotes for a grid with four levels"""
    for shift in (0.0, 0.5):
        H = MG.Hierarchy((33, 35, 1), shift=shift)
        K = H.matrix()
        km = np.linalg.eigvals(K @ H.M[0]).real
        print(f"(33, 35, 1) shift {shift}: levels {len(H.n)}, cond(K M) = {km.max() / km.min():.3f}")
        assert km.min() > 0.0
