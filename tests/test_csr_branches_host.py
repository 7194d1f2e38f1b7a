"""Every case of tests/csr_branch_cases.py on the plain-C oracle (oracle/hipk_cpu.c, oracle/hipk_cpu_complex.c) against the
longdouble references written from the header's contract: pins the oracle to an independent statement of the CSR products
and shows, before a GPU is involved, that the references stay inside the derived per-row bounds on these inputs.  Plus the
coverage assertions: the static case tables reach every instantiation of the row-tile kernels that csr_route_of can choose
(branch_of mirrors it) and every reachable per-tile cell; the unreachable cells are spelt out with the reason."""
import numpy as np
import pytest

from kernel_harness import Host
import csr_branch_cases as B

GROUPS = B.groups() + B.groups(knobs=True)


@pytest.mark.parametrize("gid,cases", GROUPS, ids=[g for g, _ in GROUPS])
def test_oracle_against_longdouble_reference(built, gid, cases):
    rep = B.run_cases(Host, cases)
    print(f"{gid}: {rep.summary()}")
    assert not rep.fails, f"{gid}: {rep.summary()}\n" + "\n".join(rep.fails[:20])


def test_what_the_oracle_cannot_tell_apart_is_named():
    assert set(B.ORACLE_SAME) == {"scaled/fin", "knobs"}
    assert sum(1 for gid, cs in GROUPS for c in cs) == len(B.CASES)            # no case is left out of a group


def _plan(c):
    return B.plan_of(c["mat"], not B.is_z(c["dt"]))


def test_case_tables_cover_every_instantiation(built):
    have = set()
    for c in B.CASES:
        have |= set(B.branch_of(c, _plan(c), c.get("knobs")))
    want = B.wanted_instantiations()
    missing = sorted(str(x) for x in want - have)
    print(f"{len(want & have)} of {len(want)} instantiations, {len(B.CASES)} cases")
    assert len(want) == 16 * 2 + 6 + 6 and not missing, f"instantiations without a case: {missing}"
    assert not have - want, sorted(str(x) for x in have - want)
    # what only an environment knob reaches is reached by that knob's cases
    plain = set()
    for c in B.CASES:
        if not c.get("knobs"):
            plain |= set(B.branch_of(c, _plan(c)))
    only_knobs = want - plain
    assert {x for x in only_knobs if x[0] == "csr_stream_kernel"} == {x for x in want if x[0] == "csr_stream_kernel" and x[4]}
    assert {x for x in only_knobs if x[0] == "csr_rows_block_kernel"} == {x for x in want if x[0] == "csr_rows_block_kernel" and x[2] == 1}
    assert {x for x in only_knobs if x[0] == "csr_window_block_kernel"} == {x for x in want if x[0] == "csr_window_block_kernel" and x[3] == "XS_MAX" and not x[4]}


def test_case_tables_cover_every_reachable_cell(built):
    cells, marks, per_kernel = set(), set(), {}
    for c in B.CASES:
        cs, ms = B.cells_of(c, _plan(c), c.get("knobs"))
        cells |= cs
        marks |= ms
        for b in B.branch_of(c, _plan(c), c.get("knobs")):
            per_kernel.setdefault(b[0], set()).update(cs)
    grid = {(a, b, s, h) for a in B.AXES[0] for b in B.AXES[1] for s in B.AXES[2] for h in B.AXES[3]}
    assert len(grid) == 24 and B.REACHABLE | set(B.UNREACHABLE) == grid and not B.REACHABLE & set(B.UNREACHABLE)
    assert len(B.REACHABLE) == 10 and all(isinstance(r, str) and r for r in B.UNREACHABLE.values())
    assert cells == B.REACHABLE, (sorted(map(str, B.REACHABLE - cells)), sorted(map(str, cells - B.REACHABLE)))
    assert not B.WANTED_MARKS - marks, sorted(map(str, B.WANTED_MARKS - marks))
    # the kernels without a window stage: gathers, one lane per row, on both kinds of slab and all three kinds of tile
    for k in ("csr_stream_kernel", "csr_rows_block_kernel", "zcsr_kernel"):
        assert per_kernel[k] == {(a, "gather", 1, h) for a in B.AXES[0] for h in B.AXES[3]}, k
    assert per_kernel["csr_window_block_kernel"] == {x for x in B.REACHABLE if x[3] == "local"}


def test_widths_and_variants_of_the_issue():
    def widths(ep, z):
        return {c["w"] for c in B.CASES if c["ep"] == ep and B.is_z(c["dt"]) == z and not c.get("rc") and not c.get("knobs")}
    assert widths("matvec", False) == {1, 2, 3, 4, 5, 8, 9, 16, 64, 65} and widths("shifted", False) == {1, 2, 5, 8, 64}
    assert widths("matvec", True) == {1, 2, 3, 5, 64, 65} and widths("shifted", True) == {1, 2, 5, 64}
    for dt in B.RTYPES + B.ZTYPES:
        for fl in B.FLAVOURS:
            mine = [c for c in B.CASES if c["dt"] == dt and c["flavour"] == fl and not c.get("knobs")]
            declined = {(c["mat"], c["w"], bool(c.get("noshift"))) for c in mine if c["ep"] == "shifted" and c.get("rc") == 1}
            if B.is_z(dt):
                assert declined == {("band_narrow@1000", 65, False), ("slab_both", 2, False)}
                assert any(c["ep"] == "matvec" and c["mat"] == "slab_both" and c["w"] == 65 for c in mine)
                continue
            assert {("slab_both", 2, False), ("rect_far", 2, False), ("band_narrow@97", 65, False), ("band_narrow@97", 2, True)} <= declined
            sc = [c for c in mine if c["ep"] == "scaled"]
            assert any(c.get("rc") == -1 and c.get("alias") for c in sc)
            for m in B.SCALED:
                assert {(c["norm2"], c["fin"]) for c in sc if c["mat"] == m} == {(a, f) for a in (True, False) for f in (0, 4)}
    assert len(B.KNOBS) - 1 <= 4 and all("LD_PRELOAD" not in k["env"] for k in B.KNOBS.values())


def test_matrices_are_what_the_cases_need(built):
    """the properties of the host analysis the tables rely on, asserted on the plan so that no case can drift"""
    for n, nt in ((97, 1), (827, 7), (960, 8), (1000, 9), (1930, 17)):
        Pn = B.plan_of(f"band_narrow@{n}")
        assert Pn.ntiles == nt and Pn.windowed == 1 and Pn.col16 is not None and Pn.cw_max <= 192, (n, Pn.ntiles, Pn.cw_max)
        assert np.all(np.diff(Pn.tiles)[:-1] == 120)
    G = B.plan_of("band_narrow_g")
    assert G.windowed == 1 and G.col16 is None and G.cw_max <= 192
    W = B.plan_of("band_wide")
    cw = W.win[:W.ntiles, 1]
    assert W.windowed == 1 and W.ntiles == 3 and W.cw_max == cw.max()
    assert W.cw_max * 3 <= B.XS_SMALL < W.cw_max * 9 <= B.XS_MAX < W.cw_max * 17, cw
    assert cw.max() * 9 <= B.XS_MAX < cw.min() * 17, cw      # 8 columns: every tile windowed; 16 and 64: every tile gathers
    S = B.plan_of("short_rows")
    assert S.tiles.tolist() == [0, 256, 512, 600] and S.windowed == 1 and B.matrix("short_rows").lens.max() <= 3
    X = B.plan_of("scattered")
    assert X.windowed == 0 and X.col16 is not None and X.cw_max * 3 > B.XS_SMALL and X.cw_max <= B.XS_MAX
    R, T = B.plan_of("rect_far"), B.plan_of("rect_tall")
    assert R.col16 is None and R.windowed == 0 and (R.halo_lo, R.halo_hi) == (0, 0) and T.col16 is not None and T.windowed == 1
    Rg = B.plan_of("ragged")
    nz, nr = Rg.info[:Rg.ntiles, 3] - Rg.info[:Rg.ntiles, 2], np.diff(Rg.tiles)
    assert Rg.windowed == 0 and sorted(nz[nz >= 2048].tolist()) == [2048, 2049, 4000] and np.all(nr[nz > 2048] == 1)
    empty = np.flatnonzero(nz == 0)
    assert empty[0] == 0 and empty[-1] == Rg.ntiles - 1 and np.any((empty > 0) & (empty < Rg.ntiles - 1)) and (B.matrix("ragged").lens == 0).sum() > 1300
    assert nr[-1] <= 128                                     # the last all-empty tile is short enough for the two-lane split
    assert B.plan_of("zero").ntiles == 3 and B.matrix("zero").rp[-1] == 0
    halos = {n: (B.plan_of(n).halo_lo, B.plan_of(n).halo_hi) for n in ("slab_lo", "slab_hi", "slab_both", "slab_far")}
    assert halos["slab_lo"][0] > 0 and halos["slab_lo"][1] == 0 and halos["slab_hi"][0] == 0 and halos["slab_hi"][1] > 0
    assert halos["slab_both"][0] > 900 and halos["slab_both"][1] > 1200 and B.matrix("slab_both").lens[300] == 2100 and B.plan_of("slab_both").col16 is not None
    assert halos["slab_far"] == (0, 69400) and B.plan_of("slab_far").col16 is None
    for name in ("band_narrow@1000", "ragged", "slab_both", "slab_hi"):
        assert B.plan_of(name, real=False).col16 is None
    for c in B.CASES:
        M = B.matrix(c["mat"])
        assert M.nrows <= 6000 and len(M.ci) <= 120000


def test_layouts_differ_within_a_case():
    for fl in B.FLAVOURS:
        for lens in ([600, 600, 60, 0], [700, 700, 1000, 1300], [70000, 300, 0, 0], [300, 5000, 0, 0], [600, 600, 600, 0, 69400]):
            lds = B._lds(fl, lens)
            assert len(set(lds)) == len(lds) and all(ld > n for ld, n in zip(lds, lens)) and all(ld % 2 == (fl == "odd") for ld in lds)


def test_row_bound_sees_one_wrong_term():
    """what the per-row bound is for: the last entry of one short row dropped, in a matrix whose largest row is far larger"""
    M, plan = B.matrix("ragged"), B.plan_of("ragged")
    X, lo, hi, _, _, (y, S, n) = B._inputs("matvec", B.F64, "ragged", 1, False)
    ones = np.flatnonzero(M.lens == 1)
    i = int(ones[np.argmin(np.abs(np.asarray(y[0, ones], np.float64)))])
    bad = np.asarray(y, np.float64).copy()
    bad[0, i] = 0.0
    rep = B.Report()
    B._cmp_rows(rep, "clean", B.F64, np.asarray(y, np.float64), y, S, n[None, :])
    assert not rep.fails
    B._cmp_rows(rep, "dropped", B.F64, bad, y, S, n[None, :])
    assert len(rep.fails) == 1
    assert 0 < abs(float(y[0, i])) <= 2e-4 * (1 + float(np.abs(y).max()))      # invisible to a bound of tol (1 + max |y|)


@pytest.mark.parametrize("knobs", [k for k in B.KNOBS if k])
def test_knob_cases_land_where_meant(built, knobs):
    B.check_knob_cases(knobs)
