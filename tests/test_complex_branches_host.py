"""Every case of tests/complex_branch_cases.py on the plain-C oracle (oracle/hipk_cpu_complex.c, oracle/hipk_cpu.c) against
the clongdouble references written from the header's contract: pins the oracle to an independent statement of each complex
operation (conjugated left operand, (re, im) coefficient pairs, M[q + c nx] = M(q, c), real theta) and shows, before a GPU
is involved, that the references stay inside the derived bounds on these inputs.  Plus the coverage assertions: the static
case tables reach every instantiation the host dispatch of csrc/hipk_complex.hip can choose (branch_of mirrors it)."""
import os
import re

import numpy as np
import pytest

from kernel_harness import Host
import complex_branch_cases as Z

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# the instantiations the dispatch can choose, over both types: a new one without a case fails here
NINST = {"dots": 24,           # zdots_kernel<NX, CPW>: 12 per type
         "ritz_update": 22}    # zritz_kernel<NJ, NR>: 5, zritz2_kernel<L, NVH, NWH, NRH>: 6 per type (a seventh, <4,6,5,1>, fitted exactly
#                                what <2,12,10,2> before it fits and could not be chosen: it left the dispatch with this suite)
NCELLS = {"ritz_update": 2 * (3 * 11 + 2)}       # each instantiation, staged once and in tiles; the two chunked job mixes

GROUPS = Z.groups(Z.TABLES)


@pytest.mark.parametrize("gid,cases", GROUPS, ids=[g for g, _ in GROUPS])
def test_oracle_against_longdouble_reference(built, gid, cases):
    rep = Z.run_cases(Host, cases)
    print(f"{gid}: {rep.summary()}")
    assert not rep.fails, f"{gid}: {rep.summary()}\n" + "\n".join(rep.fails[:20])


def test_cases_the_oracle_cannot_run_are_named():
    assert set(Z.ORACLE_CANNOT) == {"dots_mfma"}
    # those cases reach the oracle as plain dots cases of the same shapes
    assert not hasattr(Host().lib, "hipk_set_zdots_mfma")
    assert all(c["ep"] == "dots" and c["mfma"] for c in Z.CASES["dots_mfma"])
    assert all(Z.branch_of(dict(c, mfma=False))[0][0] == "zdots_kernel" for c in Z.CASES["dots_mfma"])


@pytest.mark.parametrize("table", Z.TABLES)
def test_case_tables_cover_every_branch(table):
    have, want, one_size = Z.coverage(table)
    missing = sorted(str(x) for x in want - have)
    print(f"{table}: {len(want & have)} of {len(want)} cells, {len(Z.CASES[table])} cases")
    assert not missing, f"{table}: {len(missing)} of {len(want)} cells have no case: {missing[:10]}"
    assert not one_size, f"{table}: instantiations that lack a row count below one pass or one that is no multiple of it: {one_size[:10]}"
    if table in NINST:
        assert len(Z.instantiations(table)) == NINST[table]
    if table in NCELLS:
        assert len(want) == NCELLS[table]
    assert max(c["m"] for c in Z.CASES[table]) <= 2000
    if table != "copy_cols":        # its thresholds are in bytes: see _copy_cases
        assert all(c["m"] in Z.ROWS for c in Z.CASES[table])
    if table in ("project", "project_mul"):
        assert all(c["m"] <= 70 for c in Z.CASES[table] if c["tot"] >= 512)


def test_ritz_tables_with_the_one_lane_knob():
    """what the child process of the device test asserts: with HIPK_Z_NO_SPLIT every case is a one-lane form or chunked"""
    have, want, one_size = Z.coverage("ritz_update", nosplit=True)
    assert not want - have and not one_size
    assert all(x[0] == "zritz_kernel" for c in Z.CASES["ritz_update"] for x in Z.branch_of(c, nosplit=True))


def test_every_form_of_the_ritz_dispatch_can_be_chosen():
    """the job mixes (V-products, W-products, residuals) of the table are not special: over all mixes up to 40 + 40 + 20 the
    mirrored dispatch chooses exactly the forms it lists, and <32,4> / <32,16> only for a chunk of a longer list"""
    single, chunked = set(), set()
    for nv in range(0, 41):
        for nw in range(0, 41, 1 if nv < 30 else 3):
            for nr in range(0, 21):
                if nv + nw + nr == 0:
                    continue
                ln = Z.zritz_launches([(Z.XV,)] * nv + [(Z.XW,)] * nw + [(Z.RES,)] * nr)
                (single if len(ln) == 1 else chunked).update(ln)
    forms = {("zritz_kernel",) + f for f in Z.ZRITZ1} | {("zritz2_kernel",) + f for f in Z.ZRITZ2_FEW + Z.ZRITZ2_ANY}
    assert single | chunked == forms
    assert forms - single == {("zritz_kernel", 32, 4), ("zritz_kernel", 32, 16)}


def test_constants_match_the_sources():
    def define(path, name):
        text = open(os.path.join(ROOT, path)).read()
        return re.search(r"#define\s+%s\s+(\w+)" % name, text).group(1)
    assert int(define("primme_amd/csrc/hipk_panel_dev.h", "UTIL_MAXCOLS")) == Z.UTIL_MAXCOLS
    assert int(define("include/primme_amd_kernels.h", "HIPK_Z_PROJECT_MAXCOEF")) == Z.ZPROJ_LDS
    assert define("primme_amd/csrc/hipk_complex.hip", "ZPROJ_LDS") == "HIPK_Z_PROJECT_MAXCOEF"
    assert all(nx in nxs and nx + 1 in nxs for nxs in (Z.COL_OPS["axpy"], Z.COL_OPS["xpay"]) for nx in (Z.UTIL_MAXCOLS,))
    assert all(Z.UTIL_MAXCOLS + 1 in Z.COL_OPS[op] for op in ("scale", "residual", "gather"))


def test_layout_flavours_and_guards():
    for dt in Z.ZTYPES:
        for m in Z.ROWS:
            ops = {f: Z.zlayout(dt, m, 3, f, extra=1) for f in Z.FLAVOURS[dt]}
            assert ops["eq"].ld == m and ops["odd"].ld > m and ops["odd"].ld % 2 == 1 and ops["even"].ld > m and ops["even"].ld % 2 == 0
            if dt == Z.C32:
                assert ops["shift"].shift == 1 and (ops["shift"].off * 8) % 16 == 8 and ops["shift"].ld > m
            for op in ops.values():
                assert op.off >= 64 and op.host.size - (op.off + 3 * op.ld) >= 64 and op.rows == m
                assert np.isnan(op.host.real).all() and np.isnan(op.host.imag).all()      # NaN in BOTH halves
    s = Z.zsmall(5, 2)
    assert s.dtype == np.complex128 and s.ld == 8 and np.isnan(s.host.imag).all()


def test_guard_check_sees_a_one_element_overrun_of_a_complex_operand():
    """a store one row past m, which with ld == m is row 0 of the next column; and one that changes only the imaginary
    half of an element (the halves are compared as separate integers)"""
    for dt in Z.ZTYPES:
        op = Z.zlayout(dt, 700, 2, "eq")
        op.fill(range(2), np.full((2, 700), 1 + 2j))
        op.expect(0)
        after = op.host.copy()
        after[op.index(0)] = 3 - 1j
        rep = Z.Report()
        rep.guard("clean", op, after)
        assert not rep.fails
        after[op.off + 700] = 3 - 1j
        rep.guard("overrun", op, after)
        assert len(rep.fails) == 1 and "column 1 row 0" in rep.fails[0]
        after = op.host.copy()
        after[op.off + 700 + 5] = complex(1, 2.5)                        # only the imaginary half of one input element
        rep = Z.Report()
        rep.guard("imaginary half", op, after)
        assert len(rep.fails) == 1 and "column 1 row 5" in rep.fails[0]
        after = op.host.copy()
        after[op.off - 1] = complex(np.nan, 0.0)                         # a guard element: NaN stays in the real half only
        rep = Z.Report()
        rep.guard("guard, imaginary half", op, after)
        assert len(rep.fails) == 1
        rep = Z.Report()
        rep.same_bits("same", op.host, op.host.copy())
        assert not rep.fails
        rep.same_bits("imaginary half", op.host, after)
        assert len(rep.fails) == 1
