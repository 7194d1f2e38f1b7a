"""Every case of tests/panel_branch_cases.py on the plain-C oracle (oracle/hipk_cpu.c) against the longdouble references
written from the header's contract: pins the oracle to an independent statement of each operation and shows, before a GPU
is involved, that the references stay inside the derived bounds on these inputs.  Plus the coverage assertions: the static
case tables reach every instantiation the host dispatch can choose (branch_of mirrors that dispatch)."""
import numpy as np
import pytest

from primme_amd import _ffi as F
from kernel_harness import Host
import panel_branch_cases as P

TABLES = ["residual", "residual_dev", "project", "project_mul", "dots", "ritz_update", "update_overlaps", "triple"]
NCELLS = {"residual": 128}


def _oracle_can(c):
    return not c.get("fin")          # P.ORACLE_CANNOT["project/fin"]; the whole table "dots_wide" is P.ORACLE_CANNOT["dots_wide"]


GROUPS = [(gid, [c for c in cs if _oracle_can(c)]) for gid, cs in P.groups(TABLES)]
GROUPS = [(gid, cs) for gid, cs in GROUPS if cs]


@pytest.mark.parametrize("gid,cases", GROUPS, ids=[g for g, _ in GROUPS])
def test_oracle_against_longdouble_reference(built, gid, cases):
    rep = P.run_cases(Host, cases)
    print(f"{gid}: {rep.summary()}")
    assert not rep.fails, f"{gid}: {rep.summary()}\n" + "\n".join(rep.fails[:20])


def test_cases_the_oracle_cannot_run_are_named():
    left_out = [c for tb in TABLES for c in P.CASES[tb] if not _oracle_can(c)]
    assert left_out and all(c["ep"] == "project" and c["fin"] for c in left_out)
    assert set(P.ORACLE_CANNOT) == {"project/fin", "dots_wide"}
    # the shapes of the left-out cases still reach the oracle: as project cases without the switch / as plain dots cases
    assert all(P.branch_of(dict(c, nomfma=False))[0] == "dots_mfma_kernel" for c in P.CASES["dots_wide"])


@pytest.mark.parametrize("table", TABLES + ["dots_wide"])
def test_case_tables_cover_every_branch(table):
    have, want, one_size = P.coverage(table)
    missing = sorted(str(x) for x in want - have)
    print(f"{table}: {len(want & have)} of {len(want)} cells, {len(P.CASES[table])} cases")
    assert not missing, f"{table}: {len(missing)} of {len(want)} cells have no case: {missing[:10]}"
    assert not one_size, f"{table}: instantiations run at one row count only: {one_size[:10]}"
    if table in NCELLS:
        assert len(want) == NCELLS[table]
    assert max(c["m"] for c in P.CASES[table]) <= 2000


def test_layout_flavours_and_guards():
    for dt in (F.HIPK_F64, F.HIPK_F32):
        w = 16 // np.dtype(P.NPDT[dt]).itemsize
        tails = set()
        for m in P.M_SMALL + P.M_LARGE + P.M_LARGE_BIGK:
            v, o, s = (P.layout(dt, m, 3, f) for f in ("vec", "odd", "shift"))
            assert P.is_vec(dt, v) and not P.is_vec(dt, o) and not P.is_vec(dt, s)
            assert o.ld % 2 == 1 and o.shift == 0 and s.shift == 1 and (s.ld * s.dtype.itemsize) % 16 == 0
            assert v.ld - m < w and (v.ld == m) == (m % w == 0)
            tails.add(m % w)
            for op in (v, o, s):
                assert op.off >= 64 and op.host.size - (op.off + 3 * op.ld) >= 64 and min(op.ld, op.rows) == m
                live = np.zeros(op.host.size, bool)
                live[op.index(range(3))] = True
                assert np.isnan(op.host).all() and live.sum() == 3 * m
        assert tails == set(range(w))            # every tail length of a 16-byte vector, and ld == m (tail 0)


def test_guard_check_sees_a_one_row_overrun():
    """what the comparison is for: a store one row past m, which with ld == m is row 0 of the next column"""
    op = P.layout(F.HIPK_F64, 716, 2, "vec")
    op.fill(range(2), np.ones((2, 716)))
    op.expect(0)
    after = op.host.copy()
    after[op.index(0)] = 2.0
    rep = P.Report()
    rep.guard("clean", op, after)
    assert not rep.fails
    after[op.off + 716] = 2.0
    rep.guard("overrun", op, after)
    assert len(rep.fails) == 1 and "column 1 row 0" in rep.fails[0]
