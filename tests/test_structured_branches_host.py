"""Every case of tests/structured_branch_cases.py on the plain-C oracle (plain CSR, hipk_stencil_create, hipk_csr_matvec_scaled;
for the Chebyshev step the oracle's product followed by the combination in numpy double) against the longdouble references
written from the header's contract, inside the derived bounds.  Plus the coverage assertions: the static case tables reach all 80
instantiations of pat_kernel, every reachable cell of its per-chunk paths (the unreachable ones are spelt out with the reason),
the six instantiations and the per-segment paths of pb_matvec_kernel; and the sensitivity of the per-row bound to the mistakes
these kernels can make, each of which a bound of tol (1 + max |y|) does not see."""
import numpy as np
import pytest

from kernel_harness import Host
import csr_branch_cases as CB
import structured_branch_cases as B

GROUPS = B.groups() + B.groups(knobs=True)


@pytest.mark.parametrize("gid,cases", GROUPS, ids=[g for g, _ in GROUPS])
def test_oracle_against_longdouble_reference(built, gid, cases):
    rep = B.run_cases(Host, cases)
    print(f"{gid}: {rep.summary()}")
    assert not rep.fails, f"{gid}: {rep.summary()}\n" + "\n".join(rep.fails[:20])


def test_what_the_oracle_cannot_tell_apart_is_named():
    assert set(B.ORACLE_SAME) == {"scaled/fin", "matvec/format", "cheb", "tail", "pb"}
    assert sum(1 for gid, cs in GROUPS for c in cs) == len(B.CASES)            # no case is left out of a group
    assert len(B.PB_KNOBS) == 3 and all("LD_PRELOAD" not in k["env"] for k in B.PB_KNOBS.values())


def test_case_tables_cover_every_instantiation():
    have = set()
    for c in B.CASES:
        if c["ep"] in ("matvec", "scaled", "tail", "cheb"):
            have |= set(B.branch_of(c))
    want = B.wanted_instantiations()
    pat = {x for x in have if x[0] == "pat_kernel"}
    print(f"{len(want & pat)} of {len(want)} instantiations of pat_kernel, {len(B.CASES)} cases")
    assert len(want) == 80 and not want - pat, sorted(map(str, want - pat))
    assert not pat - want, sorted(map(str, pat - want))
    assert have - pat == {("row tiles", "f64"), ("row tiles", "f32")}            # the declined matrices and the two-column product
    # the deferred tail runs the fused kernel, exact and diagonal-split, in both types
    tail = set()
    for c in B.CASES:
        if c["ep"] == "tail":
            tail |= {(b[1], b[5]) for b in B.branch_of(c)}
    assert tail == {(t, d) for t in ("f64", "f32") for d in ("exact", "diag")}


def test_case_tables_cover_every_reachable_cell():
    cells, marks, per = set(), set(), {}
    for m in B.PAT_MATS:
        cs, ms = B.cells_of_matrix(m)
        cells |= cs
        marks |= ms
        I = B.pat_info(m)
        per.setdefault(("halo" if I.halo else "local", "diag" if I.diag else "exact"), set()).update(cs)
    grid = {(p, a, v) for p in B.PATHS for a, vs in B.AXES.items() for v in vs}
    assert B.REACHABLE | set(B.UNREACHABLE) == grid and not B.REACHABLE & set(B.UNREACHABLE) and len(B.UNREACHABLE) == 5
    assert all(isinstance(r, str) and r for r in B.UNREACHABLE.values())
    assert cells == B.REACHABLE, (sorted(map(str, B.REACHABLE - cells)), sorted(map(str, cells - B.REACHABLE)))
    assert not B.WANTED_MARKS - marks, sorted(map(str, B.WANTED_MARKS - marks))
    # each of the four (local | halo) x (exact | diag) families of instantiations walks both paths, same and split pairs
    for fam, cs in per.items():
        assert {("inner", "pair", "same"), ("inner", "pair", "split"), ("guard", "pair", "same"), ("guard", "pair", "split"), ("guard", "clamped", True)} <= cs, fam
    assert {("guard", "source", "lo"), ("guard", "source", "hi")} <= per[("halo", "exact")] & per[("halo", "diag")]
    # every matrix of the pattern tables is run by the plain product in both types and flavours
    for dt in B.RTYPES:
        for fl in B.FLAVOURS:
            assert {c["mat"] for c in B.CASES if c["ep"] == "matvec" and c["dt"] == dt and c["flavour"] == fl and c["w"] == 1} == set(B.PAT_MATS + B.DECLINED)


def test_panel_blocked_tables_reach_every_cell():
    cells, per_u = set(), {}
    for c in B.CASES:
        if c["ep"] == "pb":
            cs = B.pb_cells(c["mat"], c["dt"], c["knobs"])
            cells |= cs
            per_u.setdefault((B.PB_KNOBS[c["knobs"]]["U"], B.TNAME[c["dt"]]), set()).update(k for (a, k) in ((x[0], x[1]) for x in cs) if a == "segment")
    print({k: sorted(v) for k, v in sorted(per_u.items())})
    assert not B.PB_WANTED - cells, sorted(map(str, B.PB_WANTED - cells))
    for kn in B.PB_KNOBS:
        ws = {(c["mat"], c["w"]) for c in B.CASES if c.get("knobs") == kn}
        assert {("pb_wide", 1), ("pb_wide", 2), ("pb_wide", 3)} <= ws                       # 1 and 2 through the form, 3 through the row tiles
    for c in B.CASES:
        if c["ep"] == "pb":
            M = B.matrix(c["mat"])
            assert M.nrows <= 6000 and M.xlen <= 6000 and len(M.ci) <= 60000


def test_variants_of_the_issue():
    for dt in B.RTYPES:
        for fl in B.FLAVOURS:
            mine = [c for c in B.CASES if c["dt"] == dt and c["flavour"] == fl and not c.get("knobs")]
            sc = [c for c in mine if c["ep"] == "scaled"]
            assert any(c.get("rc") == -1 and c.get("alias") for c in sc)
            for m in B.SCALED_MATS:
                assert {(c["norm2"], c["fin"]) for c in sc if c["mat"] == m} == {(a, f) for a in (True, False) for f in (0, 4)}
            ch = [c for c in mine if c["ep"] == "cheb"]
            assert {(c["w"], c["yprev"]) for c in ch if not c.get("rc")} == {(nx, yp) for nx in (1, 3, 8) for yp in (None, "given", "alias")}
            assert {(c["rc"], c["w"], bool(c.get("outyk"))) for c in ch if c.get("rc")} == {(-1, 1, True), (-1, 9, False), (1, 1, False)}
            st = [c for c in mine if c["ep"] == "stencil"]
            assert {c["grid"] for c in st} == {(1000,), (7, 5), (5, 4, 3), (1, 6), (1, 1, 1)} and {c["w"] for c in st} == {1, 3, 8}
            assert len([c for c in mine if c["ep"] == "tail"]) == 4 and any(c["ep"] == "matvec" and c["w"] == 2 for c in mine)
    assert {c["dt"] for c in B.CASES if c.get("rc") == -44} == {B.F.HIPK_C64, B.F.HIPK_C32}


def _paths(name):
    M, I = B.matrix(name), B.pat_info(name)
    return ["inner" if (c * 512 + 512 <= M.nrows and (not I.halo or (c * 512 + I.minoff >= 0 and c * 512 + 511 + I.maxoff < M.nrows))) else "guard"
            for c in range(I.nch)]


def test_matrices_are_what_the_cases_need():
    """the properties the tables rely on, asserted on the restatement so that no case can drift"""
    for n, nch in zip(B.LAP1D, (1, 1, 1, 1, 2, 2, 7, 8, 9, 12, 20)):
        I = B.pat_info(f"lap1d@{n}")
        assert (I.nch, I.npat, I.ml, I.minoff, I.maxoff) == (nch, min(n, 3), 3, -1 if n > 1 else 0, 1 if n > 1 else 0), n
    I = B.pat_info("lap1d@512")                               # a full chunk whose last pair is split and near
    assert _paths("lap1d@512") == ["inner"] and I.pid[510] != I.pid[511] and ("inner", "pair", "split+near") in B.cells_of_matrix("lap1d@512")[0]
    I = B.pat_info("lap1d@1024")                              # a first pair that is split and not near
    assert I.pid[0] != I.pid[1] and 512 + I.maxoff < 1024
    assert B.grid_of(20) == 16 and B.grid_of(12) == 8 and B.grid_of(1) == 8
    for L, ml in zip(range(1, 9), (3, 3, 3, 5, 5, 7, 7, 8)):
        M, I = B.matrix(f"lattice@{L}"), B.pat_info(f"lattice@{L}")
        assert M.nrows == 1537 and I.ml == ml and int(M.lens.max()) == L and not I.diag and (I.minoff, I.maxoff) == (-(L // 2), L - L // 2 - 1 if L > 1 else 0)
        assert M.lens[0] < L or L == 1
        pairs = I.pid[512:1024].reshape(-1, 2)
        assert (pairs[:, 0] == pairs[:, 1]).any() and (pairs[:, 0] != pairs[:, 1]).any()           # away from the ends
        T = B.pat_info(f"diag:lattice@{L}")
        assert T.diag and T.ml == ml and T.npat <= 2 * (L + 1)
    R = B.pat_info("ring@2048")
    assert (R.minoff, R.maxoff, R.nch) == (-2047, 2047, 4) and _paths("ring@2048") == ["inner"] * 4
    assert (B.pat_info("lap2d@32x64").ml, B.pat_info("lap2d@37x41").ml, B.pat_info("lap3d@8x8x40").ml) == (5, 5, 7)
    assert _paths("lap2d@37x41") == ["inner", "inner", "guard"] and _paths("lap3d@8x8x40") == ["inner"] * 5
    H = B.matrix("holes")
    assert (H.lens == 0).sum() > 100 and 0 in B.pat_info("holes").plen
    assert (B.pat_info("npat256").npat, B.pat_info("npat256").ml) == (256, 3) and B.pat_info("npat257") is None and B.pat_info("row9") is None
    assert int(B.matrix("row9").lens.max()) == 9
    halos = {s: (B.matrix(s).halo_lo, B.matrix(s).halo_hi) for s in B.SLABS}
    assert halos == {"slab:lattice@8/4000:1000:1536": (4, 3), "slab:lattice@2/4000:1000:1536": (1, 0), "slab:lattice@4/4000:1000:1536": (2, 1),
                     "slab:lattice@6/4000:1000:1536": (3, 2), "slab:lattice@8/4000:3700:300": (4, 0), "slab:lattice@8/4000:0:700": (0, 3),
                     "slab:lattice@8/4000:2:600": (2, 3), "slab:ring@3000:0:1100": (0, 1900), "slab:ring@3000:1000:1536": (1, 1),
                     "slab:lap2d@32x64:20:1100": (20, 32), "slab:lap2d@37x41:500:400": (37, 37), "slab:lap3d@8x8x40:640:1536": (64, 64)}, halos
    assert _paths(B.SLABS[0]) == ["guard", "inner", "guard"] == _paths("diag:" + B.SLABS[0])
    assert _paths("slab:lattice@2/4000:1000:1536") == ["guard", "inner", "inner"]                 # no entry above the slab's rows: maxoff = 0
    assert _paths("slab:lattice@8/4000:3700:300") == ["guard"] and _paths("slab:lap2d@37x41:500:400") == ["guard"]
    for t in B.TWINS:
        I = B.pat_info(t)
        assert I is not None and I.diag and I.npat <= 256, t
    assert -1 in B.pat_info("diag:nodiag:lattice@4").ds and {0, 1, 2} <= set(B.pat_info("diag:nodiag:lattice@4").ds.tolist())
    for name in B.PAT_MATS + B.DECLINED:
        assert B.matrix(name).nrows <= 10240
    # the panel-blocked plans
    assert B.pb_plan("pb_wide", B.F64, "pb")[:4] == (10, 5, 512, 2) and B.pb_plan("pb_wide", B.F32, "pb")[:4] == (11, 3, 256, 3)
    assert B.pb_plan("pb_wide", B.F64, "pb_u2_tile1")[:4] == (10, 5, 64, 11)
    assert B.pb_plan("pb_tall", B.F64, "pb_u8")[:4] == (10, 1, 2048, 3) and B.pb_plan("pb_tall", B.F32, "pb")[:4] == (11, 1, 2048, 3)
    assert B.pb_plan("pb_seg", B.F64, "pb_u2_tile1")[4].tolist() == [[512, 0, 0, 0], [507, 0, 0, 0], [5, 0, 40, 0], [0, 0, 0, 612]]
    assert B.pb_plan("pb_seg", B.F64, "pb")[4].tolist() == [[1024, 0, 40, 612]] and B.pb_plan("pb_seg", B.F32, "pb_u8")[4].tolist() == [[1024, 652]]
    assert int(B.matrix("pb_wide").lens[5]) == 300 and int(B.matrix("pb_wide").ci[B.matrix("pb_wide").rp[5]:B.matrix("pb_wide").rp[6]].max()) < 1024
    # the stencil slabs: halo below, above, both; shorter than the reach; thinner than a plane
    S = {(g, r0, m): (B.stencil_matrix(g, r0, m).halo_lo, B.stencil_matrix(g, r0, m).halo_hi) for g, r0, m in B.STENCIL}
    assert S[((5, 4, 3), 7, 40)] == (7, 13) and S[((5, 4, 3), 25, 9)] == (20, 20) and S[((5, 4, 3), 0, 20)] == (0, 20) and S[((5, 4, 3), 40, 20)] == (20, 0)
    assert S[((7, 5), 3, 20)] == (3, 7) and S[((7, 5), 16, 4)] == (7, 7) and S[((1, 6), 2, 3)] == (1, 1) and S[((1, 1, 1), 0, 1)] == (0, 0)
    assert S[((1000,), 300, 333)] == (1, 1)
    assert [B.stencil_matrix(g, 0, int(np.prod(g))).dims for g in ((1000,), (7, 5), (5, 4, 3), (1, 6), (1, 1, 1))] == [1, 2, 3, 2, 1]


def test_layouts_differ_within_a_case():
    for fl in B.FLAVOURS:
        for lens in ([1, 1, 0, 0], [1536, 1536, 4, 3], [1100, 1100, 0, 1900], [1537] * 5, [5000, 700, 0, 0]):
            lds = B._lds(fl, lens)
            assert len(set(lds)) == len(lds) and all(ld > n for ld, n in zip(lds, lens)) and all(ld % 2 == (fl == "odd") for ld in lds)


# ---- what the per-row bound is for: the mistakes these kernels can make, each invisible to tol (1 + max |y|) ----
def _sees(y, S, n, i, wrong, tol=2e-4):
    """row i replaced by `wrong`: the per-row comparison fails on exactly that row, tol (1 + max |y|) does not notice"""
    good, bad = np.asarray(y, np.float64), np.asarray(y, np.float64).copy()
    bad[0, i] = np.float64(wrong)
    rep = B.Report()
    CB._cmp_rows(rep, "clean", B.F64, good, y, S, n[None, :])
    assert not rep.fails
    CB._cmp_rows(rep, "corrupted", B.F64, bad, y, S, n[None, :])
    assert len(rep.fails) == 1 and f"flat index {i}" in rep.fails[0], rep.fails
    assert 0 < abs(bad[0, i] - good[0, i]) <= tol * (1 + float(np.abs(good).max()))


def _quiet_x(M, rows, seed):
    """random x, small where the rows under test read it: their y is small beside the largest row's"""
    x = np.random.default_rng(seed).standard_normal((1, M.xlen))
    x[0, rows] *= 1e-6
    return x


def test_row_bound_sees_a_split_pair_computed_with_the_first_rows_offsets():
    M, I = B.matrix("lattice@8"), B.pat_info("lattice@8")
    a = 2
    assert I.pid[a] != I.pid[a + 1] and I.pats[I.pid[a]][0] != I.pats[I.pid[a + 1]][0][:len(I.pats[I.pid[a]][0])]
    x = _quiet_x(M, np.arange(0, 16), 1)
    empty = np.zeros((1, 0))
    y, S, n = CB.ref_matvec(M, M, B.F64, x, empty, empty)
    offa = list(I.pats[I.pid[a]][0]) + [0] * 8
    vb = M.va[M.rp[a + 1]:M.rp[a + 2]]
    wrong = sum(B.LD(v) * B.LD(x[0, a + 1 + offa[e]]) for e, v in enumerate(vb))
    _sees(y, S, n, a + 1, wrong)


def test_row_bound_sees_the_last_column_read_as_zero():
    M = B.matrix("ring@2048")
    x = _quiet_x(M, np.array([M.nrows - 1]), 2) * np.where(np.arange(M.xlen) < 4, 1e-3, 1.0)
    empty = np.zeros((1, 0))
    y, S, n = CB.ref_matvec(M, M, B.F64, x, empty, empty)
    assert M.ci[M.rp[1] - 1] == M.nrows - 1                   # row 0 references the last column
    _sees(y, S, n, 0, y[0, 0] - B.LD(M.va[M.rp[1] - 1]) * B.LD(x[0, -1]))


def test_row_bound_sees_the_tables_zero_in_place_of_the_streamed_diagonal():
    M, I = B.matrix("diag:lattice@5"), B.pat_info("diag:lattice@5")
    x = np.random.default_rng(3).standard_normal((1, M.xlen))
    empty = np.zeros((1, 0))
    y, S, n = CB.ref_matvec(M, M, B.F64, x, empty, empty)
    d = np.zeros(M.nrows)
    on = M.ci == M.rowid
    d[M.rowid[on]] = M.va[on]
    i = int(np.argmin(np.where(d != 0, np.abs(d * x[0]), np.inf)))
    assert I.diag and I.ds[I.pid[i]] >= 0
    _sees(y, S, n, i, y[0, i] - B.LD(d[i]) * B.LD(x[0, i]))


def test_row_bound_sees_one_lost_lds_add_of_the_long_row():
    M = B.matrix("pb_wide")
    x = np.random.default_rng(4).standard_normal((1, M.xlen))
    empty = np.zeros((1, 0))
    y, S, n = CB.ref_matvec(M, M, B.F64, x, empty, empty)
    terms = M.va[M.rp[5]:M.rp[6]] * x[0, M.ci[M.rp[5]:M.rp[6]]]
    assert len(terms) == 300
    e = int(np.argmin(np.abs(terms)))
    _sees(y, S, n, 5, y[0, 5] - B.LD(M.va[M.rp[5] + e]) * B.LD(x[0, M.ci[M.rp[5] + e]]))
